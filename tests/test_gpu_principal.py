"""Principal strains on the GPU: f3d_principal_strain against its float32 restatement (tests/principal_ref.py) bit for bit, all ten
fields and the statistics, on the shapes the strain fields are tested on (tile seams x = 63 / 64, y = 3 / 4, z = 31 / 32, thin
shapes, size-1 axes, boxes inside poisoned larger containers) for smooth, affine and noisy displacements with NaN holes; the field
selection and the refusals of the entry; its agreement with f3d_flow_strain on E; the driver's principal strains of a solved flow
and of a trajectory (OpticalFlow.principal); and bin/flow3d --principal against the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import exact_ref as X
from principal_ref import NAMES, principal_of_tensor, principal_ref, principal_stats_ref
from strain_ref import same_bits
from subbox import SENTINEL_BITS, SubBox, outside, poison
from test_gpu_strain import KW, five_frames, random_displacement
from test_gpu_strain_compose_exact import SEAMS, SUB_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
GROUPS = (1, 1, 1, 2, 4, 4, 4, 8, 8, 8)
ALL = ("val", "shear", "dir1", "dir3")


def differing(a, b):
    return int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def check_stats(got, want_fields):
    want = principal_stats_ref(want_fields["e1"], want_fields["e3"], want_fields["gmax"])
    assert got["defined"] == want["defined"], (got, want)
    for k in ("e1_max", "e3_min", "shear_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("amp", [2.0, 0.05])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (37, 23, 11), (64, 64, 1), (584, 388, 5), (257, 65, 33), (128, 128, 128)])
def test_principal_strain_equals_the_restatement_bit_for_bit(f3d, dims, amp):
    """noise: every lane of a wave needs a different number of effective sweeps, which is what the early exit has to survive"""
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    u, v, ww = (c * np.float32(amp / 2.0) for c in random_displacement(rng, w, h, d))
    got = f3d.principal_strain(u, v, ww, fields=ALL)
    want = principal_ref(u, v, ww)
    for n in NAMES:
        assert same_bits(got[n], want[n]), f"{dims} {n}: {differing(got[n], want[n])} differ"
    check_stats(got["stats"], want)
    if w * h * d > 8:
        assert 0 < got["stats"]["defined"] < w * h * d
    # the instantiation that does not carry V
    vals = f3d.principal_strain(u, v, ww, fields=("val", "shear"))
    assert set(vals) == {"e1", "e2", "e3", "gmax", "stats"}
    for n in NAMES[:4]:
        assert same_bits(vals[n], want[n]), f"{dims} {n} without directions"
    check_stats(vals["stats"], want)


def test_statistics_of_a_field_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, np.float32)
    got = f3d.principal_strain(nan, nan, nan, fields=("shear",))
    st = got["stats"]
    assert st["defined"] == 0 and np.isnan(st["e1_max"]) and np.isnan(st["e3_min"]) and np.isnan(st["shear_max"])
    assert set(got) == {"gmax", "stats"} and np.isnan(got["gmax"]).all()


def run_principal(f3d, ins, outs, mask, dims, stats, null_unselected=True):
    st = f3d.PrincipalStats() if stats else None
    arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, GROUPS)]
    f3d.check(f3d._principal_entry()(*ins, (f3d._dp * 10)(*arr), mask, *dims, st), "f3d_principal_strain")
    f3d.sync()
    return None if st is None else st.as_dict()


def test_every_subset_writes_exactly_its_outputs(f3d):
    w, h, d = 70, 9, 6
    rng = np.random.default_rng(11)
    comps = random_displacement(rng, w, h, d)
    want = principal_ref(*comps)
    box = f3d.Containers(w, h, d)
    try:
        ins = [box.new(c) for c in comps]
        outs = [box.alloc() for _ in range(10)]
        box.set_current()
        for mask in range(1, 16):
            for null_unselected in (False, True):
                for p in outs:
                    f3d.check(f3d.hip().f3d_memset2d(p, box.pitch, 0x7F, box.pitch, h * d))
                st = run_principal(f3d, ins, outs, mask, (w, h, d), mask & 1, null_unselected)
                for i, (p, g) in enumerate(zip(outs, GROUPS)):
                    got = box.download(p, (w, h, d))
                    if mask & g:
                        assert same_bits(got, want[NAMES[i]]), (mask, NAMES[i])
                    else:
                        assert (got.view(np.uint32) == SENTINEL_BITS).all(), (mask, NAMES[i])
                if st is not None:
                    check_stats(st, want)
    finally:
        box.free()


@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("kind", ["affine", "smooth", "noise"])
@pytest.mark.parametrize("dims,cdims", SUB_CASES)
def test_principal_strain_of_a_box_inside_a_larger_container(f3d, dims, cdims, kind, fill):
    w, h, d = dims
    rng = np.random.default_rng(w * 131 + h * 7 + d)
    if kind == "affine":
        comps = X.affine_field(*X.STRAIN_AFFINE[1], dims)
    elif kind == "smooth":
        comps = X.smooth_displacement(dims, "sine", amp=0.2, seed=w + h + d)
    else:
        comps = [rng.uniform(-0.3, 0.3, size=(d, h, w)).astype(np.float32) for _ in range(3)]
    all_nan, one_nan = X.seam_holes(dims, rng, density=0.03)
    comps = X.with_holes(comps, all_nan, one_nan, which=0)
    und = X.predicted_undefined(all_nan | one_nan)
    want = principal_ref(*comps)
    sb = SubBox(f3d, cdims)
    try:
        ins = [sb.put(c, poison(rng, sb.full, fill)) for c in comps]
        outs = [sb.sentinel() for _ in range(10)]
        mask_out = outside(np.empty(sb.full), dims)
        for mask, stats in ((15, True), (1, False), (3, True), (4, False), (8, True), (6, False)):
            for p in outs:
                f3d.check(f3d.hip().f3d_memset2d(p, sb.c.pitch, 0x7F, sb.c.pitch, cdims[1] * cdims[2]))
            st = run_principal(f3d, ins, outs, mask, dims, stats)
            for i, (p, g) in enumerate(zip(outs, GROUPS)):
                full = sb.get(p)
                if mask & g:
                    assert (full.view(np.uint32)[mask_out] == SENTINEL_BITS).all(), (mask, NAMES[i], "written outside the box")
                    got = full[:d, :h, :w]
                    assert np.array_equal(np.isnan(got), und), (mask, NAMES[i], "undefined set")
                    assert same_bits(got, want[NAMES[i]]), (mask, NAMES[i], fill, differing(got, want[NAMES[i]]))
                else:
                    assert (full.view(np.uint32) == SENTINEL_BITS).all(), (mask, NAMES[i], "unselected output written")
            if st is not None:
                check_stats(st, want)
                assert st["defined"] == int((~und).sum())
    finally:
        sb.free()


@pytest.mark.parametrize("dims", SEAMS)
def test_principal_strain_on_the_seams_of_the_tiling(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w * 1009 + h * 101 + d)
    comps = X.smooth_displacement(dims, "quadratic", amp=0.05, seed=w + 3 * h + 7 * d)
    comps = X.with_holes(comps, *X.seam_holes(dims, rng, density=0.02), which=1)
    for x in (0, 62, 63, 64, 65, w - 1):
        for y in (0, 3, 4, h - 1):
            for z in (0, 30, 31, 32, 33, d - 1):
                if x < w and y < h and z < d and rng.random() < 0.3:
                    comps[int(rng.integers(0, 3))][z, y, x] = np.nan
    want = principal_ref(*comps)
    sb = SubBox(f3d, (w + 3, h + 2, d + 1))
    try:
        ins = [sb.put(c, poison(rng, sb.full, "finite")) for c in comps]
        outs = [sb.sentinel() for _ in range(10)]
        st = run_principal(f3d, ins, outs, 15, dims, True)
        for n, p in zip(NAMES, outs):
            full = sb.get(p)
            assert (full.view(np.uint32)[outside(full, dims)] == SENTINEL_BITS).all(), n
            assert same_bits(full[:d, :h, :w], want[n]), (n, differing(full[:d, :h, :w], want[n]))
        check_stats(st, want)
        assert st["defined"] == int((~X.predicted_undefined(X.missing_mask(*comps))).sum())
    finally:
        sb.free()


@pytest.mark.parametrize("dims", [(37, 23, 11), (130, 9, 70)])
def test_the_two_entries_agree_on_the_tensor(f3d, dims):
    """e1, e2, e3 are the eigenvalues of the very E f3d_flow_strain stores: the restatement's rules 2-4 applied to the six fields that
    entry returned on the device give the values this entry returned"""
    w, h, d = dims
    rng = np.random.default_rng(w + h + d)
    comps = random_displacement(rng, w, h, d)
    E = f3d.flow_strain(*comps, fields=("e",))
    got = f3d.principal_strain(*comps, fields=ALL)
    want = principal_of_tensor(tuple(E[n] for n in ("exx", "eyy", "ezz", "exy", "exz", "eyz")))
    und = np.isnan(E["exx"])
    assert und.any() and not und.all()
    for n in NAMES:
        assert np.array_equal(np.isnan(got[n]), und), n
        assert same_bits(got[n][~und], want[n][~und]), n


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._principal_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        p = [box.new(np.zeros((8, 8, 8), np.float32)) for _ in range(13)]
        box.set_current()
        u, v, w, outs = p[0], p[1], p[2], p[3:13]

        def call(a, b, c, o, mask):
            return fn(a, b, c, (f3d._dp * 10)(*o), mask, 8, 8, 8, None)

        bad = [
            (0, v, w, outs, 15),                                     # null input
            (u, v, 0, outs, 1),
            (u, v, w, outs[:1] + [0] + outs[2:], 1),                 # null output of a selected group
            (u, v, w, outs[:9] + [0], 8),
            (u, v, w, outs, 0),                                      # nothing selected
            (u, v, w, outs, 16),                                     # unknown bit
            (u, v, w, outs, 31),
            (u, v, w, outs[:3] + [v] + outs[4:], 2),                 # gmax output is an input
            (u, v, w, [w] + outs[1:], 1),                            # e1 output is an input
            (u, v, w, outs[:2] + [outs[0]] + outs[3:], 1),           # two values share a container
            (u, v, w, outs[:7] + [outs[4]] + outs[8:], 12),          # a d1 and a d3 component share one
        ]
        for args in bad:
            assert call(*args) != 0, args[-1]
            assert b"f3d_principal_strain" in hip.f3d_last_error()
        # the same container for an unselected output and a selected one, or an input passed as an unselected output, is fine
        assert call(u, v, w, outs[:3] + [outs[0]] + outs[4:], 1) == 0
        assert call(u, v, w, [u] * 3 + [outs[3]] + [v] * 6, 2) == 0
        f3d.sync()
    finally:
        box.free()


def test_principal_strains_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        got = flow.principal("flow", fields=ALL)
        want = principal_ref(u, v, ww)
        for n in NAMES:
            assert same_bits(got[n], want[n]), n
        check_stats(got["stats"], want)
        assert got["stats"]["defined"] == w * h * d
        part = flow.principal("flow")
        assert set(part) == {"e1", "e2", "e3", "gmax", "stats"} and all(same_bits(part[n], want[n]) for n in NAMES[:4])
        part = flow.principal("flow", fields=("dir3",))
        assert set(part) == {"d3x", "d3y", "d3z", "stats"} and all(same_bits(part[n], want[n]) for n in NAMES[7:])
        check_stats(part["stats"], want)                              # statistics need the values even when not stored
        assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, ww)))
        flow.principal_end()
        with pytest.raises(f3d.F3dError, match="trajectory"):
            flow.principal("trajectory")
        with pytest.raises(ValueError):
            flow.principal("flow", fields=("e",))
    finally:
        flow.destroy()


@pytest.fixture(scope="module")
def sequence(f3d):
    """per pair of the first four frames: the flow, the displacement, and the principal strains of both through OpticalFlow.principal"""
    dims, frames = five_frames(f3d)
    frames = frames[:4]
    flow = f3d.OpticalFlow()
    flow.initialize(*dims)
    out = []
    for k, fl, disp in flow.compute_sequence(frames, cumulative=True, **KW):
        out.append((fl, disp, flow.principal("flow", fields=ALL), flow.principal("trajectory", fields=ALL)))
    flow.destroy()
    return dims, frames, out


def test_principal_strains_between_the_yields_of_a_sequence(sequence):
    _, _, out = sequence
    assert len(out) == 3
    for k, (fl, disp, p_flow, p_traj) in enumerate(out):
        wf, wt = principal_ref(*fl), principal_ref(*disp[:3])
        for n in NAMES:
            assert same_bits(p_flow[n], wf[n]), f"pair {k} flow {n}"
            assert same_bits(p_traj[n], wt[n]), f"pair {k} trajectory {n}"
        check_stats(p_flow["stats"], wf)
        check_stats(p_traj["stats"], wt)
    assert out[-1][3]["stats"]["defined"] < out[-1][3]["e1"].size        # lost points leave undefined voxels


LINE = re.compile(r"principal frame (\d+) -> frame (\d+): e1 max (\S+), e3 min (\S+), shear max (\S+), (\d+) undefined of (\d+) voxels")


def check_line(m, stats, a, b, total):
    assert (int(m[0]), int(m[1])) == (a, b)
    assert int(m[5]) == total - stats["defined"] and int(m[6]) == total
    for txt, val in ((m[2], stats["e1_max"]), (m[3], stats["e3_min"]), (m[4], stats["shear_max"])):
        assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


def test_cli_principal_equals_the_binding(sequence, tmp_path):
    (w, h, d), frames, out = sequence
    total = w * h * d
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(np.float32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent"]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), np.float32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()
    strain_names = ("vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq")
    strain_line = re.compile(r"^strain frame .*$", re.M)

    def run(tag, frames_, extra):
        r = subprocess.run(args + ["--frames", *frames_, "--out", str(tmp_path / tag)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    # cumulative, with --strain beside it: the principal strains of the displacement frame 0 -> frame k+1
    so = run("cp", paths, ["--cumulative", "--strain", "vol,e,eq", "--principal", "val,shear,dir1,dir3"])
    ss = run("cs", paths, ["--cumulative", "--strain", "vol,e,eq"])
    lines = LINE.findall(so)
    assert len(lines) == 3 and not LINE.findall(ss)
    assert strain_line.findall(so) == strain_line.findall(ss) and len(strain_line.findall(ss)) == 3
    for k in range(3):
        for n in NAMES:
            assert same_bits(read(f"cp_{k}_principal-{n}{suffix}"), out[k][3][n]), f"cumulative {k} {n}"
        for n in strain_names:                                         # --strain's files do not change
            assert raw(f"cp_{k}_strain-{n}{suffix}") == raw(f"cs_{k}_strain-{n}{suffix}"), f"strain {k} {n}"
        for c in "uvw":
            assert raw(f"cp_{k}_flow-{c}{suffix}") == raw(f"cs_{k}_flow-{c}{suffix}"), f"flow {k} {c}"
            assert raw(f"cp_{k}_disp-{c}{suffix}") == raw(f"cs_{k}_disp-{c}{suffix}"), f"disp {k} {c}"
        check_line(lines[k], out[k][3]["stats"], 0, k + 1, total)
    assert not any(n.startswith("cs_") and "principal" in n for n in os.listdir(tmp_path))

    # without --cumulative: of each pair's flow, only the selected groups
    so = run("fp", paths, ["--principal", "val,dir3"])
    lines = LINE.findall(so)
    assert len(lines) == 3 and not strain_line.findall(so)
    for k in range(3):
        for n in NAMES:
            name = f"fp_{k}_principal-{n}{suffix}"
            if n in ("e1", "e2", "e3", "d3x", "d3y", "d3z"):
                assert same_bits(read(name), out[k][2][n]), f"flow {k} {n}"
            else:
                assert not os.path.exists(tmp_path / name)
        for c in "uvw":
            assert raw(f"fp_{k}_flow-{c}{suffix}") == raw(f"cs_{k}_flow-{c}{suffix}"), f"flow {k} {c}"
        check_line(lines[k], out[k][2]["stats"], k, k + 1, total)
    assert not any(n.startswith("fp_") and "strain" in n for n in os.listdir(tmp_path))

    # one pair, computed synchronously: tag without the pair index
    so = run("one", paths[:2], ["--principal", "shear", "--cumulative"])
    lines = LINE.findall(so)
    assert len(lines) == 1
    for n in NAMES:
        name = f"one_principal-{n}{suffix}"
        if n == "gmax":
            assert same_bits(read(name), out[0][3][n])
        else:
            assert not os.path.exists(tmp_path / name)
    check_line(lines[0], out[0][3]["stats"], 0, 1, total)
    so = run("onef", paths[:2], ["--principal", "dir1", "--strain", "eq"])
    for n in ("d1x", "d1y", "d1z"):
        assert same_bits(read(f"onef_principal-{n}{suffix}"), out[0][2][n]), n
    check_line(LINE.findall(so)[0], out[0][2]["stats"], 0, 1, total)
    assert os.path.exists(tmp_path / f"onef_strain-eq{suffix}") and len(strain_line.findall(so)) == 1
