"""Strain fields on the GPU: f3d_flow_strain against its float32 restatement (tests/strain_ref.py) bit for bit with its statistics,
the field selection and the refusals of the entry, the driver's strain of a solved flow and of a trajectory (OpticalFlow.strain),
a there-and-back sequence whose Lagrangian strain vanishes, and bin/flow3d --strain against the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from strain_ref import NAMES, same_bits, strain_ref, strain_stats_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
SENTINEL = 0x7F      # byte fill of unselected outputs: 0x7F7F7F7F = 3.39e38


def random_displacement(rng, w, h, d):
    """smooth-ish random displacement with a NaN hole (all three components), scattered lost points and a few voxels with one
    NaN component"""
    shape = (d, h, w)
    comps = [rng.uniform(-2, 2, size=shape).astype(np.float32) for _ in range(3)]
    pick = rng.random(shape)
    lost = pick < 0.04
    z0, y0, x0 = (int(rng.integers(0, n)) for n in shape)
    lost[z0:z0 + max(1, d // 4), y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 4)] = True
    for c in comps:
        c[lost] = np.nan
    comps[1][(pick > 0.5) & (pick < 0.51)] = np.nan
    return comps


def check_stats(got, vol, eq):
    want = strain_stats_ref(vol, eq)
    for k in ("defined", "folded"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("vol_min", "vol_max", "eq_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])
    scale = max(1.0, float(np.nansum(np.abs(vol.astype(np.float64)))))
    assert abs(got["vol_sum"] - want["vol_sum"]) <= 1e-9 * scale, (got["vol_sum"], want["vol_sum"])


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (37, 23, 11), (64, 64, 1), (584, 388, 5), (257, 65, 33), (128, 128, 128)])
def test_flow_strain_equals_the_restatement_bit_for_bit(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    u, v, ww = random_displacement(rng, w, h, d)
    got = f3d.flow_strain(u, v, ww)
    want = strain_ref(u, v, ww)
    for n in NAMES:
        assert same_bits(got[n], want[n]), f"{dims} {n}: {int(np.sum(~((got[n] == want[n]) | (np.isnan(got[n]) & np.isnan(want[n])))))} differ"
    check_stats(got["stats"], want["vol"], want["eq"])
    if w * h * d > 8:
        assert 0 < got["stats"]["defined"] < w * h * d and got["stats"]["folded"] > 0


def test_statistics_of_a_field_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, np.float32)
    got = f3d.flow_strain(nan, nan, nan, fields=("vol",))
    st = got["stats"]
    assert st["defined"] == 0 and st["folded"] == 0 and st["vol_sum"] == 0
    assert np.isnan(st["vol_min"]) and np.isnan(st["vol_max"]) and np.isnan(st["eq_max"])
    assert set(got) == {"vol", "stats"} and np.isnan(got["vol"]).all()


MASKS = {"vol": 1, "e": 2, "eq": 4}


def test_every_subset_writes_exactly_its_outputs(f3d):
    w, h, d = 70, 9, 6
    rng = np.random.default_rng(11)
    comps = random_displacement(rng, w, h, d)
    want = strain_ref(*comps)
    fn = f3d._strain_entry()
    box = f3d.Containers(w, h, d)
    try:
        ins = [box.new(c) for c in comps]
        outs = [box.alloc() for _ in range(8)]
        box.set_current()
        groups = [1, 2, 2, 2, 2, 2, 2, 4]
        for mask in range(1, 8):
            for null_unselected in (False, True):
                for p in outs:
                    f3d.check(f3d.hip().f3d_memset2d(p, box.pitch, SENTINEL, box.pitch, h * d))
                arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, groups)]
                stats = f3d.StrainStats() if mask & 1 else None
                f3d.check(fn(*ins, (f3d._dp * 8)(*arr), mask, w, h, d, stats), "f3d_flow_strain")
                f3d.sync()
                for i, (p, g) in enumerate(zip(outs, groups)):
                    got = box.download(p, (w, h, d))
                    if mask & g:
                        assert same_bits(got, want[NAMES[i]]), (mask, NAMES[i])
                    else:
                        assert (got.view(np.uint32) == 0x7F7F7F7F).all(), (mask, NAMES[i])
                if stats is not None:
                    check_stats({k: getattr(stats, k) for k, _ in stats._fields_}, want["vol"], want["eq"])
    finally:
        box.free()


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._strain_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        p = [box.new(np.zeros((8, 8, 8), np.float32)) for _ in range(11)]
        box.set_current()
        u, v, w, outs = p[0], p[1], p[2], p[3:11]

        def call(a, b, c, o, mask):
            return fn(a, b, c, (f3d._dp * 8)(*o), mask, 8, 8, 8, None)

        bad = [
            (0, v, w, outs, 7),                                      # null input
            (u, v, w, outs[:1] + [0] + outs[2:], 2),                 # null output of a selected group
            (u, v, w, outs, 0),                                      # nothing selected
            (u, v, w, outs, 8),                                      # unknown bit
            (u, v, w, outs[:7] + [v], 4),                            # eq output is an input
            (u, v, w, [w] + outs[1:], 1),                            # vol output is an input
            (u, v, w, outs[:3] + [outs[1]] + outs[4:], 2),           # two E outputs share a container
            (u, v, w, outs[:7] + [outs[0]], 5),                      # vol and eq share one
        ]
        for args in bad:
            assert call(*args) != 0, args[-1]
            assert b"f3d_flow_strain" in hip.f3d_last_error()
        # the same container for an unselected output and a selected one, or an input passed as an unselected output, is fine
        assert call(u, v, w, outs[:7] + [outs[0]], 1) == 0
        assert call(u, v, w, [u] * 7 + [outs[7]], 4) == 0
        f3d.sync()
    finally:
        box.free()


def test_strain_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        got = flow.strain("flow")
        want = strain_ref(u, v, ww)
        for n in NAMES:
            assert same_bits(got[n], want[n]), n
        check_stats(got["stats"], want["vol"], want["eq"])
        assert got["stats"]["defined"] == w * h * d
        part = flow.strain("flow", fields=("eq",))
        assert set(part) == {"eq", "stats"} and same_bits(part["eq"], want["eq"])
        check_stats(part["stats"], want["vol"], want["eq"])          # statistics need vol and eq even when not stored
        assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, ww)))
        flow.strain_end()
        with pytest.raises(f3d.F3dError, match="trajectory"):
            flow.strain("trajectory")
    finally:
        flow.destroy()


def five_frames(f3d):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    i128 = np.load(os.path.join(ROOT, "tests", "golden", "inputs_128.npz"))
    crop = (slice(40, 40 + d), slice(40, 40 + h), slice(40, 40 + w))
    c0 = i128["frame_0"].astype(np.float32)[crop].copy()
    c1 = i128["frame_1"].astype(np.float32)[crop].copy()
    return (w, h, d), [s0, s1, c1, c0, s0]


@pytest.fixture(scope="module")
def sequence(f3d):
    """per pair of the first four frames: the flow, the displacement, and the strain of both through OpticalFlow.strain"""
    dims, frames = five_frames(f3d)
    frames = frames[:4]
    flow = f3d.OpticalFlow()
    flow.initialize(*dims)
    out = []
    for k, fl, disp in flow.compute_sequence(frames, cumulative=True, **KW):
        out.append((fl, disp, flow.strain("flow"), flow.strain("trajectory")))
    flow.destroy()
    return dims, frames, out


def test_strain_between_the_yields_of_a_sequence(sequence):
    _, _, out = sequence
    assert len(out) == 3
    for k, (fl, disp, s_flow, s_traj) in enumerate(out):
        wf, wt = strain_ref(*fl), strain_ref(*disp[:3])
        for n in NAMES:
            assert same_bits(s_flow[n], wf[n]), f"pair {k} flow {n}"
            assert same_bits(s_traj[n], wt[n]), f"pair {k} trajectory {n}"
        check_stats(s_flow["stats"], wf["vol"], wf["eq"])
        check_stats(s_traj["stats"], wt["vol"], wt["eq"])
    assert out[-1][3]["stats"]["defined"] < out[-1][3]["vol"].size        # lost points leave undefined voxels


def test_there_and_back_has_no_lagrangian_strain(f3d):
    """[f0, f1, f0] of the synthetic pair: after the second pair the points are home, so the strain of the displacement is near 0
    in the interior"""
    S = 64
    f0, f1 = f3d.synth_pair(S, S, S)
    flow = f3d.OpticalFlow()
    flow.initialize(S, S, S)
    kw = dict(warp_levels_count=24, outer_iterations_count=10)
    res = []
    for k, _, disp in flow.compute_sequence([f0, f1, f0], cumulative=True, **kw):
        res.append(flow.strain("trajectory"))
    flow.destroy()
    core = (slice(16, 48),) * 3
    st = res[1]
    home = ~np.isnan(st["vol"][core])
    assert home.mean() > 0.99
    vol = np.abs(st["vol"][core][home])
    e = max(float(np.abs(st[n][core][home]).mean()) for n in NAMES[1:7])
    print(f"there and back: mean |vol| {vol.mean():.4g}, max mean |E_ij| {e:.4g}, eq mean {float(st['eq'][core][home].mean()):.4g}")
    assert vol.mean() < 0.05 and e < 0.05
    assert st["stats"]["folded"] == 0


LINE = re.compile(r"strain frame (\d+) -> frame (\d+): vol min/mean/max (\S+)/(\S+)/(\S+), eq max (\S+), (\d+) folded, "
                  r"(\d+) undefined of (\d+) voxels")


def check_line(m, stats, a, b, total):
    assert (int(m[0]), int(m[1])) == (a, b)
    assert int(m[6]) == stats["folded"] and int(m[7]) == total - stats["defined"] and int(m[8]) == total
    mean = stats["vol_sum"] / stats["defined"]
    for txt, val in ((m[2], stats["vol_min"]), (m[3], mean), (m[4], stats["vol_max"]), (m[5], stats["eq_max"])):
        assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


def test_cli_strain_equals_the_binding(sequence, tmp_path):
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

    def run(tag, frames_, extra):
        r = subprocess.run(args + ["--frames", *frames_, "--out", str(tmp_path / tag)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    # cumulative: the Lagrangian strain of the displacement frame 0 -> frame k+1
    so = run("cs", paths, ["--cumulative", "--strain", "vol,e,eq"])
    run("c", paths, ["--cumulative"])
    lines = LINE.findall(so)
    assert len(lines) == 3
    for k in range(3):
        for n in NAMES:
            assert same_bits(read(f"cs_{k}_strain-{n}{suffix}"), out[k][3][n]), f"cumulative {k} {n}"
        for c in "uvw":
            assert raw(f"cs_{k}_flow-{c}{suffix}") == raw(f"c_{k}_flow-{c}{suffix}"), f"flow {k} {c}"
            assert raw(f"cs_{k}_disp-{c}{suffix}") == raw(f"c_{k}_disp-{c}{suffix}"), f"disp {k} {c}"
        check_line(lines[k], out[k][3]["stats"], 0, k + 1, total)
    assert not any(n.startswith("c_") and "strain" in n for n in os.listdir(tmp_path))

    # without --cumulative: the strain of each pair's flow, only the selected groups
    so = run("fs", paths, ["--strain", "vol,eq"])
    run("f", paths, [])
    lines = LINE.findall(so)
    assert len(lines) == 3
    for k in range(3):
        for n in NAMES:
            name = f"fs_{k}_strain-{n}{suffix}"
            if n in ("vol", "eq"):
                assert same_bits(read(name), out[k][2][n]), f"flow {k} {n}"
            else:
                assert not os.path.exists(tmp_path / name)
        for c in "uvw":
            assert raw(f"fs_{k}_flow-{c}{suffix}") == raw(f"f_{k}_flow-{c}{suffix}"), f"flow {k} {c}"
        check_line(lines[k], out[k][2]["stats"], k, k + 1, total)

    # one pair, computed synchronously: tag without the pair index
    so = run("one", paths[:2], ["--strain", "e", "--cumulative"])
    lines = LINE.findall(so)
    assert len(lines) == 1
    for n in NAMES:
        name = f"one_strain-{n}{suffix}"
        if n in ("vol", "eq"):
            assert not os.path.exists(tmp_path / name)
        else:
            assert same_bits(read(name), out[0][3][n]), n
    check_line(lines[0], out[0][3]["stats"], 0, 1, total)
    so = run("onef", paths[:2], ["--strain", "vol"])
    assert same_bits(read(f"onef_strain-vol{suffix}"), out[0][2]["vol"])
    check_line(LINE.findall(so)[0], out[0][2]["stats"], 0, 1, total)
