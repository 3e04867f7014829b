"""Trajectory accumulation on the GPU: f3d_compose_flow against its float32 restatement (tests/trajectory_ref.py) bit for bit, the
sequence API of the binding (OpticalFlow.compute_sequence, trajectory_*) against fresh solves and the restatement, a there-and-back
sequence that must come home, and bin/flow3d --cumulative against the binding."""
import os
import subprocess

import numpy as np
import pytest

from trajectory_ref import compose_ref, compose_sequence_ref, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)


def random_step(rng, w, h, d):
    """acc with small and large displacements (points leaving through every face), NaN, and positions exactly on 0 and W-1 / H-1
    / D-1; inc of a few voxels"""
    shape = (d, h, w)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    acc = [rng.uniform(-2, 2, size=shape).astype(np.float32) for _ in range(3)]
    pick = rng.random(shape)
    for a, n in zip(acc, (w, h, d)):
        big = pick < 0.15
        a[big] = rng.uniform(-0.7 * n - 2, 0.7 * n + 2, size=int(big.sum())).astype(np.float32)
    for a, c, n in zip(acc, (x, y, z), (w, h, d)):
        lo = (pick > 0.5) & (pick < 0.55)
        hi = (pick > 0.55) & (pick < 0.6)
        a[lo] = -c[lo].astype(np.float32)                 # position exactly 0
        a[hi] = (n - 1 - c[hi]).astype(np.float32)        # position exactly n - 1
    acc[1][(pick > 0.97) & (pick < 0.98)] = np.nan
    inc = [rng.uniform(-3, 3, size=shape).astype(np.float32) for _ in range(3)]
    return acc, inc


@pytest.mark.parametrize("dims", [(1, 1, 1), (37, 23, 11), (64, 64, 1), (584, 388, 5), (257, 65, 33), (128, 128, 128)])
def test_compose_flow_equals_the_restatement_bit_for_bit(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    acc, inc = random_step(rng, w, h, d)
    *got, lost = f3d.compose_flow(acc, inc)
    want = compose_ref(acc, inc)
    for g, e, n in zip(got, want, "uvw"):
        assert same_bits(g, e), f"{dims} {n}: {np.sum(~((g == e) | (np.isnan(g) & np.isnan(e))))} voxels differ"
    assert lost == int(np.isnan(got[0]).sum())
    if w * h * d > 1:
        assert 0 < lost < w * h * d
    # a second step from there: lost points stay lost, the count does not shrink
    *again, lost2 = f3d.compose_flow(got, inc)
    for g, e in zip(again, compose_ref(got, inc)):
        assert same_bits(g, e)
    assert lost2 == int(np.isnan(again[0]).sum()) >= lost


def test_compose_flow_refuses_an_increment_that_is_the_accumulator(f3d):
    hip = f3d.hip()
    box = f3d.Containers(8, 8, 8)
    p = [box.new(np.zeros((8, 8, 8), np.float32)) for _ in range(4)]
    box.set_current()
    fn = f3d._compose_entry()
    try:
        assert fn(p[0], p[1], p[2], p[3], p[0], p[3], 8, 8, 8, None) != 0
        assert b"f3d_compose_flow" in hip.f3d_last_error()
        assert fn(p[0], p[1], p[2], p[3], p[3], p[3], 8, 8, 8, None) == 0     # one flow for all three components is fine
        f3d.check(hip.f3d_stream_sync())
    finally:
        box.free()


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
    dims, frames = five_frames(f3d)
    flow = f3d.OpticalFlow()
    flow.initialize(*dims)
    out = list(flow.compute_sequence(frames, cumulative=True, **KW))
    plain = list(flow.compute_sequence(frames, **KW))
    flow.destroy()
    return dims, frames, out, plain


def test_sequence_flows_equal_fresh_solves(f3d, sequence):
    dims, frames, out, plain = sequence
    assert [k for k, _, _ in out] == [0, 1, 2, 3] and all(disp is None for _, _, disp in plain)
    for (k, flow, _), (_, flow_plain, _) in zip(out, plain):
        fresh = f3d.OpticalFlow()
        fresh.initialize(*dims)
        want = fresh.compute(frames[k], frames[k + 1], silent=True, **KW)
        fresh.destroy()
        for g, p, e, n in zip(flow, flow_plain, want, "uvw"):
            assert same_bits(g, e) and same_bits(p, e), f"pair {k} {n}"


def test_sequence_displacement_equals_the_restatement(sequence):
    _, _, out, _ = sequence
    want = compose_sequence_ref([flow for _, flow, _ in out])
    for (k, flow, disp), e in zip(out, want):
        *dsp, lost = disp
        for g, x, n in zip(dsp, e, "uvw"):
            assert same_bits(g, x), f"displacement after pair {k}, {n}"
        assert lost == int(np.isnan(dsp[0]).sum())
    first = out[0][2]
    for g, f in zip(first[:3], out[0][1]):
        assert np.array_equal(g, f)       # == : the first step gives the flow back, -0 as +0
    assert out[-1][2][3] > 0              # the crops and the synthetic pair do not match: some points leave


def test_there_and_back_comes_home(f3d):
    """[f0, f1, f0] of the synthetic pair (shift (2, -1, 0.5)): after the first pair the interior moved by about the shift, after
    the second it is back.  Measured on the MI355X: after pair 1 the interior mean is (1.970, -0.990, 0.498); after pair 2 every
    interior voxel is still inside and the mean |displacement| there is 0.021 x the mean |f_0| (bounds below with margin)."""
    S = 64
    f0, f1 = f3d.synth_pair(S, S, S)
    flow = f3d.OpticalFlow()
    flow.initialize(S, S, S)
    kw = dict(warp_levels_count=24, outer_iterations_count=10)
    out = list(flow.compute_sequence([f0, f1, f0], cumulative=True, **kw))
    flow.destroy()
    core = (slice(16, 48),) * 3
    u1, v1, w1, _ = out[0][2]
    means = (float(u1[core].mean()), float(v1[core].mean()), float(w1[core].mean()))
    assert abs(means[0] - 2.0) < 0.2 and abs(means[1] + 1.0) < 0.1 and abs(means[2] - 0.5) < 0.05, means
    u2, v2, w2, lost = out[1][2]
    mag0 = np.sqrt(u1[core] ** 2 + v1[core] ** 2 + w1[core] ** 2)
    mag2 = np.sqrt(u2[core] ** 2 + v2[core] ** 2 + w2[core] ** 2)
    home = ~np.isnan(mag2)
    assert home.mean() > 0.99
    ratio = float(mag2[home].mean() / mag0.mean())
    assert ratio <= 0.25, (ratio, means)


def test_cli_cumulative_equals_the_binding(f3d, sequence, tmp_path):
    (w, h, d), frames, out, _ = sequence
    paths = []
    for i, f in enumerate(frames[:4]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(np.float32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--frames", *paths, "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent"]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), np.float32).reshape(d, h, w)
    run = subprocess.run(args + ["--out", str(tmp_path / "cum"), "--cumulative"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.count("voxels have left the volume") == 3
    plain = subprocess.run(args + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert "left the volume" not in plain.stdout
    for k in range(3):
        for i, c in enumerate("uvw"):
            got = read(f"cum_{k}_disp-{c}{suffix}")
            assert same_bits(got, out[k][2][i]), f"disp {k} {c}"
            a = open(tmp_path / f"cum_{k}_flow-{c}{suffix}", "rb").read()
            assert a == open(tmp_path / f"plain_{k}_flow-{c}{suffix}", "rb").read(), f"flow {k} {c}"
    assert not any(n.startswith("plain") and "disp" in n for n in os.listdir(tmp_path))
    for extra in (["--partial"], ["--concurrent", "2"]):
        bad = subprocess.run(args + ["--out", str(tmp_path / "bad"), "--cumulative"] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--cumulative" in bad.stdout, extra
