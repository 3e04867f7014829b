"""Local correlation without a GPU: the numpy restatement (tests/correlation_ref.py, the checker of f3d_local_correlation) on inputs
whose answer is known, the weak link of the host library, the argument errors of flow3d --match, the symbols of both headers and the
binding's names.

Bounds.  The sums are binary64 and the tail is three float32 roundings of values near 1 (two square roots and a product in the
denominator, one division), so |zncc - 1| of perfectly correlated volumes is a few float32 ulps (2^-23 = 1.19e-7).  BOUND is four times
the worst the restatement shows on the seeded inputs below, 2.39e-7 (two ulps) on 70 x 24 x 20 uniform noise in [0, 255] at
r = 1 .. 4, with and without holes; the figure stands in DESIGN.md section 14.  The kernel itself gets no tolerance at all
(tests/test_gpu_correlation.py compares it with the restatement bit for bit)."""
import ctypes as C
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from correlation_ref import local_correlation, window_sums
from inverse_ref import carry_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
BOUND = 4 * 2.39e-7
RADII = (1, 2, 3, 4)
CONSTANTS = (0.1, 1 / 3, 255.3, 1e-3, 6.5e4, -7.77, 1e-20, 3e12)


def noise(seed, shape):
    return np.random.default_rng(seed).uniform(0, 255, shape).astype(F32)


@pytest.fixture(scope="module")
def volumes():
    """70 x 24 x 20 uniform noise, and the same with 5 % NaN voxels and a NaN block"""
    a = noise(20261017, (20, 24, 70))
    holes = a.copy()
    holes[np.random.default_rng(7).random(a.shape) < 0.05] = np.nan
    holes[5:9, 6:12, 20:30] = np.nan
    return {"plain": a, "holes": holes}


# ---- perfectly correlated volumes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("which", ["plain", "holes"])
def test_a_volume_against_itself_and_against_an_affine_copy(volumes, which, r):
    a = volumes[which]
    present = ~np.isnan(a)
    for b, name in ((a, "itself"), ((F32(1.7) * a + F32(40)).astype(F32), "1.7 a + 40")):
        zncc, rmsd, st = local_correlation(a, b, r)
        assert np.array_equal(np.isnan(rmsd), ~present) and not np.isnan(zncc[present]).any()   # noise is nowhere flat
        assert np.isnan(zncc[~present]).all()
        worst = float(np.abs(zncc[present].astype(np.float64) - 1).max())
        print(f"{which} r={r} against {name}: worst |zncc - 1| {worst:.3g}")
        assert worst <= BOUND, worst
        assert st["defined"] == int(present.sum()) and st["lost"] == int((~present).sum()) and st["below"] == 0
        if b is a:
            assert (rmsd[present] == 0).all() and st["rmsd_max"] == 0.0
        else:
            assert (rmsd[present] > 0).all()


@pytest.mark.parametrize("r", RADII)
def test_constant_volumes_are_flat_everywhere(r):
    shape = (9, 10, 11)
    worst = 0.0
    for c in CONSTANTS:
        v = np.full(shape, c, F32)
        zncc, rmsd, st = local_correlation(v, v, r)
        assert np.isnan(zncc).all() and (rmsd == 0).all(), c
        assert st["defined"] == 0 and st["lost"] == 0 and np.isnan(st["zncc_min"]) and st["zncc_sum"] == 0.0
        _, (n, Sa, _, Saa, _, _, _) = window_sums(v, v, r)
        worst = max(worst, float((np.abs(n * Saa - Sa * Sa) / (n * Saa)).max()))
    print(f"r={r}: worst |va| / (n Saa) of a constant volume {worst:.3g} (the floor is 2^-40 = {2.0 ** -40:.3g})")
    assert worst < 2.0 ** -40 / 100
    # two constants: rmsd is their difference to rounding (binary64 sums of equal terms, one float32 division and square root)
    for ca, cb in ((0.1, 255.3), (1 / 3, -7.77), (6.5e4, 1e-3)):
        va, vb = np.full(shape, ca, F32), np.full(shape, cb, F32)
        zncc, rmsd, _ = local_correlation(va, vb, r)
        diff = abs(float(F32(ca)) - float(F32(cb)))
        assert np.isnan(zncc).all() and np.abs(rmsd.astype(np.float64) - diff).max() <= 4 * np.spacing(F32(diff)), (ca, cb)


def test_a_small_ripple_on_a_large_mean_is_not_flat():
    v = (1000 + 0.01 * np.random.default_rng(3).choice([-1.0, 1.0], (9, 10, 11))).astype(F32)
    zncc, _, st = local_correlation(v, v, 2)
    assert st["defined"] == v.size and np.abs(zncc.astype(np.float64) - 1).max() <= BOUND


# ---- uncorrelated volumes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_independent_noise_has_the_spread_of_a_sample_correlation(r):
    """The correlation of N = (2r+1)^3 independent pairs has mean 0 and standard deviation 1 / sqrt(N - 1), which is (2r+1)^-3/2 to
    1.9 % at r = 1 and closer above.  Neighbouring windows overlap, so the interior of one 70 x 24 x 24 volume holds only
    62 * 16 * 16 / 729 = 22 independent windows at r = 4 and its standard deviation scatters by some 15 % from draw to draw, more
    than the 10 % asked of it; twelve independent volumes of that size are pooled, which brings the scatter to about 4 %."""
    inner = []
    for seed in range(12):
        a, b = noise(100 + 2 * seed, (24, 24, 70)), noise(101 + 2 * seed, (24, 24, 70))
        zncc, _, _ = local_correlation(a, b, r)
        inner.append(zncc[r:-r, r:-r, r:-r].astype(np.float64).ravel())
    inner = np.concatenate(inner)
    expect = (2 * r + 1) ** -1.5
    print(f"r={r}: mean {inner.mean():.4f}, std {inner.std():.5f} against (2r+1)^-3/2 = {expect:.5f} ({inner.std() / expect - 1:+.1%})")
    assert abs(inner.mean()) <= 0.02
    assert abs(inner.std() / expect - 1) <= 0.10


# ---- a shifted volume ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", (1, 3))
def test_the_right_displacement_registers_a_shifted_volume(r):
    """frame 1 is frame 0 moved by (3, -2, 1) voxels; carried back through that displacement it is frame 0 wherever the point stays
    inside, and through the zero displacement it is not"""
    big = noise(5, (30, 34, 50))
    sx, sy, sz = 3, -2, 1
    f0 = big[4:24, 4:28, 4:44]
    f1 = big[4 - sz:24 - sz, 4 - sy:28 - sy, 4 - sx:44 - sx]       # f1(x + s) = f0(x)
    right = [np.full(f0.shape, s, F32) for s in (sx, sy, sz)]
    zero = [np.zeros(f0.shape, F32)] * 3
    warped, lost = carry_ref(f1, *right, "linear")
    assert 0 < lost < f0.size
    zncc, rmsd, st = local_correlation(f0, warped, r)
    defined = ~np.isnan(zncc)
    assert st["lost"] == lost and defined.sum() == f0.size - lost
    assert np.abs(zncc[defined].astype(np.float64) - 1).max() <= BOUND and (rmsd[defined] == 0).all()
    unregistered, _ = carry_ref(f1, *zero, "linear")
    z0, _, _ = local_correlation(f0, unregistered, r)
    assert np.nanmean(z0[defined]) < np.nanmean(zncc[defined]) - 0.5


# ---- edges of the definition -----------------------------------------------------------------------------------------------------------------

def test_window_larger_than_the_volume_size_one_axes_and_an_absent_centre():
    a, b = noise(21, (2, 3, 4)), noise(22, (2, 3, 4))
    zncc, rmsd, _ = local_correlation(a, b, 4)                      # every window holds the whole volume: one value everywhere
    A, B = a.astype(np.float64), b.astype(np.float64)
    assert np.ptp(zncc) <= 2 * np.spacing(F32(1)) and abs(float(zncc[0, 0, 0]) - np.corrcoef(A.ravel(), B.ravel())[0, 1]) <= 1e-6
    assert np.abs(rmsd - np.sqrt(np.mean((A - B) ** 2))).max() <= 1e-4
    # size-1 axes: the window degenerates to a line, then to the voxel itself (a single sample is flat)
    line_a, line_b = noise(23, (1, 1, 9)), noise(24, (1, 1, 9))
    zncc, rmsd, _ = local_correlation(line_a, line_b, 1)
    x = 4
    want = np.corrcoef(line_a[0, 0, x - 1:x + 2].astype(np.float64), line_b[0, 0, x - 1:x + 2].astype(np.float64))[0, 1]
    assert abs(float(zncc[0, 0, x]) - want) <= 1e-6
    zncc, rmsd, st = local_correlation(line_a[:, :, :1], line_b[:, :, :1], 2)
    assert np.isnan(zncc).all() and st["defined"] == 0 and st["lost"] == 0
    assert float(rmsd[0, 0, 0]) == pytest.approx(abs(float(line_a[0, 0, 0]) - float(line_b[0, 0, 0])), rel=1e-6)
    # an absent centre is NaN in both outputs and counts as lost; its neighbours leave it out of their sums
    c = noise(25, (5, 5, 5))
    d = c.copy()
    d[2, 2, 2] = np.nan
    zncc, rmsd, st = local_correlation(c, d, 1)
    assert np.isnan(zncc[2, 2, 2]) and np.isnan(rmsd[2, 2, 2]) and st["lost"] == 1 and st["defined"] == c.size - 1
    _, (n, *_) = window_sums(c, d, 1)
    assert n[2, 2, 1] == 26 and n[0, 0, 0] == 8 and n[2, 2, 2] == 26


# ---- the weak link of the host library ---------------------------------------------------------------------------------------------------

CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    u, v, w = flow.download()
    for call in (lambda: flow.match(), lambda: flow.match(fields="warped", radius=1), lambda: pkg.local_correlation(f0, f1)):
        try:
            call(); raise SystemExit("a call succeeded without f3d_local_correlation")
        except pkg.F3dError as e:
            assert "f3d_local_correlation" in str(e), str(e)
    host = pkg.host()
    ptrs = (pkg._fp * 3)(*[np.empty((D, H, W), np.float32).ctypes.data_as(pkg._fp) for _ in range(3)])
    assert host.f3d_flow_match_compute(flow._h, 0, 7, 3, 0.8, ptrs, None) != 0
    assert b"f3d_local_correlation" in host.f3d_host_last_error()
    flow.match_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_local_correlation: libf3d_host.so built against it must still load (RTLD_NOW) and solve,
    and local_correlation, OpticalFlow.match and f3d_flow_match_compute must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_local_correlation" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- flow3d --match --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,needle", [(["--match", "zncc,ncc"], "usage"), (["--match", "zncc,,rmsd"], "usage"),
                                          (["--match", ""], "usage"), (["--match"], "usage"),
                                          (["--match", "zncc", "--match-radius"], "usage"),
                                          (["--match", "zncc", "--match-radius", "5"], "usage"),
                                          (["--match", "zncc", "--match-radius", "0"], "usage"),
                                          (["--match-radius", "2"], "--match-radius needs --match"),
                                          (["--match", "zncc", "--partial"], "--match"),
                                          (["--match", "warped,rmsd", "--concurrent", "2"], "--match")])
def test_flow3d_match_argument_errors(tmp_path, extra, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout and "[--match warped,zncc,rmsd [--match-radius R]]" in run.stdout
    assert not any("match" in n or "flow-" in n for n in os.listdir(tmp_path))


# ---- the headers and the binding -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_local_correlation"]),
                                              ("f3d_host.h", "host", ["f3d_flow_match_compute", "f3d_flow_match_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    assert not [n for n in have if not hasattr(handle, n)]
    text = open(os.path.join(ROOT, "include", header)).read()
    if header == "f3d.h":                                      # the definition stands in the header in full
        for needle in ("q7 = (A - B)*(A - B)", "0x1p-40 * (n*Saa)", "rmsd = sqrtf((float)Sdd / (float)n)", "F3D_CORRELATION_ZNCC 1u",
                       "F3D_CORRELATION_RMSD 2u", "unsigned long long defined, lost, below;", "no running add / subtract sums"):
            assert needle in text, needle


def test_the_binding_names_the_outputs_in_abi_order(f3d):
    assert f3d.MATCH_NAMES == ("warped", "zncc", "rmsd")
    assert f3d.MATCH_GROUPS == {"warped": 1, "zncc": 2, "rmsd": 4} and f3d.CORRELATION_GROUPS == {"zncc": 1, "rmsd": 2}
    assert [n for n, _ in f3d.CorrelationStats._fields_] == ["defined", "lost", "below", "zncc_min", "rmsd_max", "zncc_sum"]
    assert C.sizeof(f3d.CorrelationStats) == 40 and f3d.CorrelationStats.zncc_sum.offset == 32
    fn = f3d._correlation_entry()
    assert len(fn.argtypes) == 10 and fn.argtypes[3] is C.c_uint and fn.argtypes[4] is C.c_uint and fn.argtypes[5] is C.c_float
    sig = inspect.signature(f3d.local_correlation)
    assert sig.parameters["radius"].default == 3 and sig.parameters["threshold"].default == 0.8
    assert sig.parameters["fields"].default == ("zncc", "rmsd")
    sig = inspect.signature(f3d.OpticalFlow.match)
    assert sig.parameters["radius"].default == 3 and sig.parameters["threshold"].default == 0.8
    assert hasattr(f3d.OpticalFlow, "match_end")
    with pytest.raises(ValueError):
        f3d._mask("zncc,ncc", f3d.MATCH_GROUPS, "match")
