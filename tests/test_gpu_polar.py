"""Local rotation and principal stretches on the GPU: f3d_polar_decomposition against its float32 restatement (tests/polar_ref.py) bit
for bit, all seven fields and the statistics (theta_sum to the last bit: the order of the reduction is fixed and restated), on the
shapes the strain fields are tested on (tile seams x = 63 / 64, y = 3 / 4, z = 31 / 32, thin shapes, size-1 axes, boxes inside
poisoned larger containers) for folding noise, small noise, and noise on a large rigid rotation, with NaN holes; the field selection
and the refusals of the entry; its agreement with f3d_principal_strain's device output; the driver's rotation of a solved flow and of
a trajectory (OpticalFlow.rotation); and bin/flow3d --rotation against the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import exact_ref as X
from polar_ref import NAMES, polar_ref, polar_stats_ref
from strain_ref import same_bits
from subbox import SENTINEL_BITS, SubBox, outside, poison
from test_gpu_strain import KW, five_frames, random_displacement
from test_gpu_strain_compose_exact import SUB_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
GROUPS = (1, 2, 2, 2, 4, 4, 4)
ALL = ("angle", "vector", "stretch")
SHAPES = [(1, 1, 1), (2, 2, 2), (37, 23, 11), (64, 64, 1), (584, 388, 5), (257, 65, 33)]
F32 = np.float32


def differing(a, b):
    return int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def check_stats(got, want_fields, folded):
    want = polar_stats_ref(want_fields, folded)
    assert got["defined"] == want["defined"] and got["folded"] == want["folded"], (got, want)
    for k in ("theta_max", "l1_max", "l3_min"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or F32(got[k]) == F32(want[k]), (k, got[k], want[k])
    assert np.float64(got["theta_sum"]).view(np.uint64) == np.float64(want["theta_sum"]).view(np.uint64), (got["theta_sum"], want["theta_sum"])
    return want


def rigid_rotation(dims, angle, axis):
    """the displacement (Q - I)(p - centre) of a rotation by `angle` about `axis` through the box centre, float32 [z, y, x]"""
    w, h, d = dims
    n = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    Q = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    z, y, x = np.meshgrid(*(np.arange(k, dtype=np.float64) for k in (d, h, w)), indexing="ij")
    p = [x - (w - 1) / 2, y - (h - 1) / 2, z - (d - 1) / 2]
    return [sum((Q[r][c] - (r == c)) * p[c] for c in range(3)).astype(F32) for r in range(3)]


def displacement(kind, dims):
    """the three inputs of the shape tests: noise of amplitude 2 (folds), of amplitude 0.05, and the latter on a rotation of 0.6 rad"""
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    amp = 2.0 if kind == "folding" else 0.05
    comps = [c * F32(amp / 2.0) for c in random_displacement(rng, w, h, d)]
    if kind == "rotated":
        comps = [c + r for c, r in zip(comps, rigid_rotation(dims, 0.6, (2.0, -3.0, 6.0)))]
    return comps


@pytest.fixture(scope="module")
def reference():
    """the restatement of every (kind, dims) of the shape tests, computed once"""
    cache = {}

    def get(kind, dims):
        if (kind, dims) not in cache:
            comps = displacement(kind, dims)
            cache[(kind, dims)] = (comps,) + polar_ref(*comps)
        return cache[(kind, dims)]

    return get


@pytest.mark.parametrize("kind", ["folding", "small", "rotated"])
@pytest.mark.parametrize("dims", SHAPES)
def test_polar_decomposition_equals_the_restatement_bit_for_bit(f3d, reference, dims, kind):
    w, h, d = dims
    comps, want, folded = reference(kind, dims)
    got = f3d.polar_decomposition(*comps, fields=ALL)
    assert set(got) == set(NAMES) | {"stats"}
    for n in NAMES:
        assert same_bits(got[n], want[n]), f"{dims} {kind} {n}: {differing(got[n], want[n])} differ"
    st = check_stats(got["stats"], want, folded)
    if w * h * d > 8:
        assert 0 < st["defined"] < w * h * d
        if kind == "folding":
            assert 0 < got["stats"]["folded"]
        if kind == "rotated" and min(dims) > 1:
            assert 0.5 < got["stats"]["theta_sum"] / st["defined"] < 0.7 and got["stats"]["theta_max"] > 0.6
    # the instantiation that carries no V: the stretches alone, without statistics
    alone = run_polar(f3d, comps, 4, stats=False)
    for n in NAMES[4:]:
        assert same_bits(alone[n], want[n]), f"{dims} {kind} {n} without the rotation"
    # the stretches alone with statistics: the angle is still reduced
    part = f3d.polar_decomposition(*comps, fields=("stretch",))
    assert set(part) == {"l1", "l2", "l3", "stats"} and all(same_bits(part[n], want[n]) for n in NAMES[4:])
    check_stats(part["stats"], want, folded)


def run_polar(f3d, comps, mask, stats):
    """the entry itself on volumes from anywhere: dict name -> array of the selected outputs (and "stats" when asked)"""
    d, h, w = comps[0].shape
    box = f3d.Containers(w, h, d)
    try:
        ins = [box.new(c) for c in comps]
        outs = [box.alloc() if mask & g else 0 for g in GROUPS]
        box.set_current()
        st = f3d.PolarStats() if stats else None
        f3d.check(f3d._polar_entry()(*ins, (f3d._dp * 7)(*outs), mask, w, h, d, st), "f3d_polar_decomposition")
        f3d.sync()
        res = {n: box.download(o, (w, h, d)) for n, o in zip(NAMES, outs) if o}
        if stats:
            res["stats"] = st.as_dict()
        return res
    finally:
        box.free()


def test_statistics_of_a_field_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, F32)
    got = f3d.polar_decomposition(nan, nan, nan, fields=("angle",))
    st = got["stats"]
    assert st["defined"] == 0 and st["folded"] == 0 and st["theta_sum"] == 0
    assert np.isnan(st["theta_max"]) and np.isnan(st["l1_max"]) and np.isnan(st["l3_min"])
    assert set(got) == {"theta", "stats"} and np.isnan(got["theta"]).all()


def call_polar(f3d, ins, outs, mask, dims, stats, null_unselected=True):
    st = f3d.PolarStats() if stats else None
    arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, GROUPS)]
    f3d.check(f3d._polar_entry()(*ins, (f3d._dp * 7)(*arr), mask, *dims, st), "f3d_polar_decomposition")
    f3d.sync()
    return None if st is None else st.as_dict()


def test_every_subset_writes_exactly_its_outputs(f3d):
    w, h, d = 70, 9, 6
    rng = np.random.default_rng(11)
    comps = [c * F32(0.5) for c in random_displacement(rng, w, h, d)]
    want, folded = polar_ref(*comps)
    assert folded.any() and not np.isnan(want["l1"]).all()
    box = f3d.Containers(w, h, d)
    try:
        ins = [box.new(c) for c in comps]
        outs = [box.alloc() for _ in range(7)]
        box.set_current()
        for mask in range(1, 8):
            for null_unselected in (False, True):
                for stats in (False, True):
                    for p in outs:
                        f3d.check(f3d.hip().f3d_memset2d(p, box.pitch, 0x7F, box.pitch, h * d))
                    st = call_polar(f3d, ins, outs, mask, (w, h, d), stats, null_unselected)
                    for i, (p, g) in enumerate(zip(outs, GROUPS)):
                        got = box.download(p, (w, h, d))
                        if mask & g:
                            assert same_bits(got, want[NAMES[i]]), (mask, stats, NAMES[i])
                        else:
                            assert (got.view(np.uint32) == SENTINEL_BITS).all(), (mask, stats, NAMES[i])
                    if st is not None:
                        check_stats(st, want, folded)
    finally:
        box.free()


@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("kind", ["affine", "smooth", "noise"])
@pytest.mark.parametrize("dims,cdims", SUB_CASES)
def test_polar_decomposition_of_a_box_inside_a_larger_container(f3d, dims, cdims, kind, fill):
    w, h, d = dims
    rng = np.random.default_rng(w * 131 + h * 7 + d)
    if kind == "affine":
        comps = X.affine_field(*X.STRAIN_AFFINE[1], dims)
    elif kind == "smooth":
        comps = X.smooth_displacement(dims, "sine", amp=0.2, seed=w + h + d)
    else:
        comps = [rng.uniform(-0.3, 0.3, size=(d, h, w)).astype(F32) for _ in range(3)]
    all_nan, one_nan = X.seam_holes(dims, rng, density=0.03)
    comps = X.with_holes(comps, all_nan, one_nan, which=0)
    und = X.predicted_undefined(all_nan | one_nan)
    want, folded = polar_ref(*comps)
    assert not (folded & und).any()
    sb = SubBox(f3d, cdims)
    try:
        ins = [sb.put(c, poison(rng, sb.full, fill)) for c in comps]
        outs = [sb.sentinel() for _ in range(7)]
        mask_out = outside(np.empty(sb.full), dims)
        for mask, stats in ((7, True), (4, False), (1, False), (2, True), (4, True), (5, False)):
            for p in outs:
                f3d.check(f3d.hip().f3d_memset2d(p, sb.c.pitch, 0x7F, sb.c.pitch, cdims[1] * cdims[2]))
            st = call_polar(f3d, ins, outs, mask, dims, stats)
            for i, (p, g) in enumerate(zip(outs, GROUPS)):
                full = sb.get(p)
                if mask & g:
                    assert (full.view(np.uint32)[mask_out] == SENTINEL_BITS).all(), (mask, NAMES[i], "written outside the box")
                    got = full[:d, :h, :w]
                    assert np.array_equal(np.isnan(got), und | folded), (mask, NAMES[i], "undefined set")
                    assert same_bits(got, want[NAMES[i]]), (mask, NAMES[i], fill, differing(got, want[NAMES[i]]))
                else:
                    assert (full.view(np.uint32) == SENTINEL_BITS).all(), (mask, NAMES[i], "unselected output written")
            if st is not None:
                check_stats(st, want, folded)
                assert st["defined"] + st["folded"] == int((~und).sum())
    finally:
        sb.free()


@pytest.mark.parametrize("dims", [(37, 23, 11), (130, 9, 70)])
def test_the_stretches_are_the_roots_of_the_device_principal_strains(f3d, dims):
    """l_i = sqrtf(2 e_i + 1) of the e_i f3d_principal_strain returned on the device, by bits, wherever the voxel is defined and not
    folded: both entries diagonalise the same tensor by the same text, and the root is monotone"""
    w, h, d = dims
    rng = np.random.default_rng(w + h + d)
    comps = [c * F32(0.25) for c in random_displacement(rng, w, h, d)]
    e = f3d.principal_strain(*comps, fields=("val",))
    got = f3d.polar_decomposition(*comps, fields=("stretch",))
    und = np.isnan(e["e1"])
    bad = np.isnan(got["l1"])
    assert und.any() and not bad.all() and (bad | ~und).all() and (bad & ~und).sum() == got["stats"]["folded"]
    with np.errstate(invalid="ignore"):
        for ln, en in (("l1", "e1"), ("l2", "e2"), ("l3", "e3")):
            assert same_bits(got[ln][~bad], np.sqrt(F32(2) * e[en][~bad] + F32(1))), ln


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._polar_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        p = [box.new(np.zeros((8, 8, 8), F32)) for _ in range(10)]
        box.set_current()
        u, v, w, outs = p[0], p[1], p[2], p[3:10]

        def call(a, b, c, o, mask):
            return fn(a, b, c, (f3d._dp * 7)(*o), mask, 8, 8, 8, None)

        bad = [
            (0, v, w, outs, 7),                                      # null input
            (u, 0, w, outs, 4),
            (u, v, 0, outs, 1),
            ([0] + outs[1:], 1),                                     # null output of a selected group
            (outs[:2] + [0] + outs[3:], 2),
            (outs[:6] + [0], 4),
            (outs, 0),                                               # nothing selected
            (outs, 8),                                               # unknown bit
            (outs, 15),
            ([v] + outs[1:], 1),                                     # theta output is an input
            (outs[:5] + [u] + outs[6:], 4),                          # l2 output is an input
            (outs[:2] + [outs[1]] + outs[3:], 2),                    # two vector components share a container
            (outs[:4] + [outs[0]] + outs[5:], 5),                    # theta and l1 share one
        ]
        for args in bad:
            args = args if len(args) == 5 else (u, v, w) + args
            assert call(*args) != 0, args[-1]
            assert b"f3d_polar_decomposition" in hip.f3d_last_error()
        assert fn(u, v, w, None, 7, 8, 8, 8, None) != 0              # no output array at all
        assert b"f3d_polar_decomposition" in hip.f3d_last_error()
        # the same container for an unselected output and a selected one, or an input passed as an unselected output, is fine
        assert call(u, v, w, outs[:4] + [outs[0]] + outs[5:], 1) == 0
        assert call(u, v, w, [u] * 4 + outs[4:], 4) == 0
        f3d.sync()
    finally:
        box.free()


@pytest.fixture(scope="module")
def sequence(f3d):
    """per pair of the first four frames: the flow, the displacement, and the rotation of both through OpticalFlow.rotation"""
    dims, frames = five_frames(f3d)
    frames = frames[:4]
    flow = f3d.OpticalFlow()
    flow.initialize(*dims)
    out = []
    for k, fl, disp in flow.compute_sequence(frames, cumulative=True, **KW):
        out.append((fl, disp, flow.rotation("flow", fields=ALL), flow.rotation("trajectory", fields=ALL)))
        part = flow.rotation("trajectory", fields=("vector",))      # the trajectory ends with the sequence: asked between the yields
    assert set(part) == {"rx", "ry", "rz", "stats"}
    flow.rotation_end()
    with pytest.raises(ValueError):
        flow.rotation("flow", fields=("val",))
    flow.destroy()
    return dims, frames, out, part


def test_rotation_between_the_yields_of_a_sequence(f3d, sequence):
    """OpticalFlow.rotation(source="flow" | "trajectory") against polar_decomposition of the downloaded displacement"""
    _, _, out, part = sequence
    assert len(out) == 3
    for k, (fl, disp, r_flow, r_traj) in enumerate(out):
        for got, src in ((r_flow, fl), (r_traj, disp[:3])):
            want = f3d.polar_decomposition(*src, fields=ALL)
            for n in NAMES:
                assert same_bits(got[n], want[n]), f"pair {k} {n}"
            for key, val in want["stats"].items():
                assert got["stats"][key] == val or (np.isnan(got["stats"][key]) and np.isnan(val)), (k, key)
            ref, folded = polar_ref(*src)
            check_stats(got["stats"], ref, folded)
    assert out[-1][3]["stats"]["defined"] < out[-1][3]["theta"].size          # lost points leave undefined voxels
    assert all(same_bits(part[n], out[-1][3][n]) for n in ("rx", "ry", "rz"))


LINE = re.compile(r"rotation frame (\d+) -> frame (\d+): angle max (\S+) rad, mean (\S+) rad, stretch max (\S+), min (\S+), (\d+) folded, "
                  r"(\d+) undefined of (\d+) voxels")


def check_line(m, stats, a, b, total):
    assert (int(m[0]), int(m[1])) == (a, b)
    assert int(m[6]) == stats["folded"] and int(m[7]) == total - stats["defined"] - stats["folded"] and int(m[8]) == total
    mean = stats["theta_sum"] / stats["defined"]
    for txt, val in ((m[2], stats["theta_max"]), (m[3], mean), (m[4], stats["l1_max"]), (m[5], stats["l3_min"])):
        assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


def test_cli_rotation_equals_the_binding(sequence, tmp_path):
    (w, h, d), frames, out, _ = sequence
    total = w * h * d
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent"]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), F32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()
    other_line = re.compile(r"^(?:strain|principal) frame .*$", re.M)

    def run(tag, extra):
        r = subprocess.run(args + ["--frames", *paths, "--out", str(tmp_path / tag)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    # cumulative, beside --strain and --principal: the rotation of the displacement frame 0 -> frame k+1
    so = run("cr", ["--cumulative", "--strain", "vol", "--principal", "val", "--rotation", "angle,vector,stretch"])
    ss = run("cs", ["--cumulative", "--strain", "vol", "--principal", "val"])
    lines = LINE.findall(so)
    assert len(lines) == 3 and not LINE.findall(ss)
    assert other_line.findall(so) == other_line.findall(ss) and len(other_line.findall(ss)) == 6
    assert so.index("principal frame 0 -> frame 1") < so.index("rotation frame 0 -> frame 1")     # after the principal strains
    for k in range(3):
        for n in NAMES:
            assert same_bits(read(f"cr_{k}_rotation-{n}{suffix}"), out[k][3][n]), f"cumulative {k} {n}"
        check_line(lines[k], out[k][3]["stats"], 0, k + 1, total)
    theirs = sorted(n for n in os.listdir(tmp_path) if n.startswith("cs_"))
    assert len(theirs) == 3 * (3 + 3 + 1 + 3) and not any("rotation" in n for n in theirs)
    for n in theirs:                                                        # the other options' files do not change
        assert raw(n) == raw("cr_" + n[3:]), n
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("cr_") and "rotation" not in n) == ["cr_" + n[3:] for n in theirs]

    # alone, without --cumulative: of each pair's flow
    so = run("fr", ["--rotation", "angle,vector,stretch"])
    lines = LINE.findall(so)
    assert len(lines) == 3 and not other_line.findall(so)
    for k in range(3):
        for n in NAMES:
            assert same_bits(read(f"fr_{k}_rotation-{n}{suffix}"), out[k][2][n]), f"flow {k} {n}"
        for c in "uvw":
            assert raw(f"fr_{k}_flow-{c}{suffix}") == raw(f"cs_{k}_flow-{c}{suffix}"), f"flow {k} {c}"
        check_line(lines[k], out[k][2]["stats"], k, k + 1, total)
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("fr_")) == sorted(
        [f"fr_{k}_rotation-{n}{suffix}" for k in range(3) for n in NAMES] + [f"fr_{k}_flow-{c}{suffix}" for k in range(3) for c in "uvw"])
