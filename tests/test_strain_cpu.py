"""Strain fields without a GPU: the float32 restatement (tests/strain_ref.py, the checker of f3d_flow_strain) against closed forms
and on its missing-sample rules, the host library's weak link to the device entry (built against a device library that lacks
f3d_flow_strain it still loads and solves, and every strain call fails with a message naming the entry), and the argument errors
of flow3d --strain, which are found before any device is touched."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from strain_ref import NAMES, fields_of_gradient, gradient_ref, strain_ref, strain_stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32


def grid(shape):
    """x, y, z coordinates (float64) of a [z, y, x] grid"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return x, y, z


def affine(A, b, shape):
    """d = A x + b in float32 (exact for the dyadic A, b and grids used here)"""
    x, y, z = grid(shape)
    d = [A[r][0] * x + A[r][1] * y + A[r][2] * z + b[r] for r in range(3)]
    out = [c.astype(F32) for c in d]
    assert all(np.array_equal(o.astype(np.float64), c) for o, c in zip(out, d))
    return out


def closed_form(A):
    """float64 vol, E, eq of a constant gradient A"""
    A = np.asarray(A, np.float64)
    vol = np.linalg.det(np.eye(3) + A) - 1
    E = 0.5 * (A + A.T + A.T @ A)
    dev = E - np.trace(E) / 3 * np.eye(3)
    eq = np.sqrt(2.0 / 3.0 * np.sum(dev * dev))
    return {"vol": vol, "exx": E[0, 0], "eyy": E[1, 1], "ezz": E[2, 2], "exy": E[0, 1], "exz": E[0, 2], "eyz": E[1, 2], "eq": eq}


@pytest.mark.parametrize("seed,shape", [(1, (17, 23, 29)), (2, (64, 5, 7)), (3, (3, 64, 2)), (4, (2, 2, 2))])
def test_affine_displacement_gives_its_matrix_everywhere(seed, shape):
    rng = np.random.default_rng(seed)
    A = rng.integers(-15, 16, size=(3, 3)) / 64.0
    b = rng.integers(-64, 65, size=3) / 16.0
    d = affine(A, b, shape)
    G, defined = gradient_ref(*d)
    assert defined.all()
    for r in range(3):
        for c in range(3):
            assert np.array_equal(G[r][c], np.full(shape, A[r][c], F32)), (r, c)   # faces included
    got = strain_ref(*d)
    one = fields_of_gradient([[np.full((1,), A[r][c], F32) for c in range(3)] for r in range(3)])
    cf = closed_form(A)
    for n in NAMES:
        assert np.array_equal(got[n], np.full(shape, one[n][0], F32)), n
        assert abs(float(one[n][0]) - cf[n]) < 1e-6, (n, float(one[n][0]), cf[n])


def rotation(deg_a, deg_b):
    a, b = np.radians(deg_a), np.radians(deg_b)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return rz @ rx


@pytest.mark.parametrize("shape", [(48, 48, 48), (64, 40, 24)])
def test_a_rigid_rotation_has_no_green_lagrange_strain(shape):
    """10 degrees about x, then 10 about z, about the centre: E and J - 1 stay at float32 rounding level (a float32 sketch gave about
    8e-7 at 48^3), while the small-strain tensor 1/2 (G + G^T) is of the order of the rotation"""
    R = rotation(10.0, 10.0)
    x, y, z = grid(shape)
    ctr = [(n - 1) / 2 for n in (shape[2], shape[1], shape[0])]
    p = [x - ctr[0], y - ctr[1], z - ctr[2]]
    d = [sum((R[r][c] - (r == c)) * p[c] for c in range(3)).astype(F32) for r in range(3)]
    got = strain_ref(*d)
    for n in NAMES:
        assert not np.isnan(got[n]).any()
        assert float(np.abs(got[n]).max()) < 1e-5, (n, float(np.abs(got[n]).max()))
    G, _ = gradient_ref(*d)
    small = max(float(np.abs(0.5 * (G[r][c] + G[c][r])).max()) for r in range(3) for c in range(3))
    assert small > 1e-2


def test_faces_take_one_sided_differences():
    rng = np.random.default_rng(5)
    shape = (4, 5, 6)
    d = [rng.uniform(-1, 1, size=shape).astype(F32) for _ in range(3)]
    G, defined = gradient_ref(*d)
    assert defined.all()
    u = d[0]
    assert np.array_equal(G[0][0][:, :, 0], u[:, :, 1] - u[:, :, 0])
    assert np.array_equal(G[0][0][:, :, -1], u[:, :, -1] - u[:, :, -2])
    assert np.array_equal(G[0][0][:, :, 2], (u[:, :, 3] - u[:, :, 1]) * F32(0.5))
    assert np.array_equal(G[0][1][:, 0, :], u[:, 1, :] - u[:, 0, :])
    assert np.array_equal(G[0][2][-1], u[-1] - u[-2])


@pytest.mark.parametrize("shape", [(1, 64, 64), (5, 388, 584), (3, 1, 9), (1, 1, 1)])
def test_an_axis_of_size_one_has_a_zero_column(shape):
    rng = np.random.default_rng(sum(shape))
    d = [rng.uniform(-1, 1, size=shape).astype(F32) for _ in range(3)]
    G, defined = gradient_ref(*d)
    assert defined.all()
    for c, axis in enumerate((2, 1, 0)):
        for r in range(3):
            if shape[axis] == 1:
                assert not G[r][c].any() and not np.signbit(G[r][c]).any()
            else:
                assert not np.isnan(G[r][c]).any()
    out = strain_ref(*d)
    assert not any(np.isnan(out[n]).any() for n in NAMES)


def test_the_rim_of_a_nan_hole_takes_one_sided_differences():
    rng = np.random.default_rng(6)
    shape = (7, 8, 9)
    d = [rng.uniform(-1, 1, size=shape).astype(F32) for _ in range(3)]
    d[1][3, 4, 4] = np.nan                     # one component is enough to lose the point
    G, defined = gradient_ref(*d)
    assert not defined[3, 4, 4] and defined.sum() == d[0].size - 1
    u = d[0]
    assert np.array_equal(G[0][0][3, 4, 5], u[3, 4, 6] - u[3, 4, 5])          # only q
    assert np.array_equal(G[0][0][3, 4, 3], u[3, 4, 3] - u[3, 4, 2])          # only m
    assert np.array_equal(G[0][1][3, 5, 4], u[3, 6, 4] - u[3, 5, 4])
    assert np.array_equal(G[0][2][2, 4, 4], u[2, 4, 4] - u[1, 4, 4])
    assert np.array_equal(G[0][0][3, 5, 5], (u[3, 5, 6] - u[3, 5, 4]) * F32(0.5))   # diagonal neighbours do not matter
    out = strain_ref(*d)
    for n in NAMES:
        assert np.isnan(out[n][3, 4, 4]) and np.isnan(out[n]).sum() == 1


def test_a_voxel_isolated_along_one_axis_is_undefined():
    rng = np.random.default_rng(7)
    shape = (6, 6, 6)
    d = [rng.uniform(-1, 1, size=shape).astype(F32) for _ in range(3)]
    d[2][2, 3, 1] = np.nan
    d[0][2, 3, 3] = np.nan                     # (2, 3, 2) has no x neighbour left, but y and z ones
    d[0][0, 5, 1] = np.nan                     # (0, 5, 0) and (2, 3, 0): a face on one side, a hole on the other
    out = strain_ref(*d)
    want = np.zeros(shape, bool)
    for p in ((2, 3, 1), (2, 3, 3), (2, 3, 2), (2, 3, 0), (0, 5, 1), (0, 5, 0)):
        want[p] = True
    for n in NAMES:
        assert np.array_equal(np.isnan(out[n]), want), n


def test_a_nan_centre_is_undefined_even_with_every_neighbour():
    shape = (5, 5, 5)
    d = [np.zeros(shape, F32) for _ in range(3)]
    d[0][2, 2, 2] = np.nan
    out = strain_ref(*d)
    assert np.isnan(out["vol"][2, 2, 2]) and np.isnan(out["vol"]).sum() == 1
    assert not out["vol"][~np.isnan(out["vol"])].any()


def test_a_local_fold_is_counted():
    """u(x) = x-compression of slope -1.5 over a band of columns: J = 1 + du/dx < 0 there, and only there"""
    shape = (6, 7, 20)
    x, _, _ = grid(shape)
    slope = np.where((x >= 8) & (x <= 11), -1.5, 0.0)
    u = np.cumsum(slope, axis=2).astype(F32)
    zero = np.zeros(shape, F32)
    out = strain_ref(u, zero, zero)
    G, _ = gradient_ref(u, zero, zero)
    st = strain_stats_ref(out["vol"], out["eq"])
    want = int((out["vol"] <= F32(-1)).sum())
    assert st["folded"] == want > 0 and st["defined"] == u.size
    assert np.array_equal(out["vol"] <= -1, G[0][0] <= -1)          # vol = du/dx exactly when the other columns are 0
    assert st["vol_min"] == float(out["vol"].min()) <= -1.5 + 1e-6
    assert st["vol_sum"] == pytest.approx(float(out["vol"].astype(np.float64).sum()))
    none = strain_stats_ref(np.full(shape, np.nan, F32), np.full(shape, np.nan, F32))
    assert none["defined"] == 0 and none["vol_sum"] == 0 and np.isnan(none["vol_min"]) and np.isnan(none["eq_max"])


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
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    for call in (lambda: flow.strain("flow"), lambda: flow.strain("flow", fields=("vol",)),
                 lambda: pkg.flow_strain(u, v, w)):
        try:
            call(); raise SystemExit("a strain call succeeded without f3d_flow_strain")
        except pkg.F3dError as e:
            assert "f3d_flow_strain" in str(e), str(e)
    # the C API itself, without the binding in between
    host = pkg.host()
    ptrs = (pkg._fp * 8)(*[np.empty((D, H, W), np.float32).ctypes.data_as(pkg._fp) for _ in range(8)])
    assert host.f3d_flow_strain_compute(flow._h, 0, 7, ptrs, None) != 0
    assert b"f3d_flow_strain" in host.f3d_host_last_error()
    try:
        flow.strain("trajectory"); raise SystemExit("strain of a trajectory that was never started succeeded")
    except pkg.F3dError as e:
        assert "trajectory" in str(e), str(e)
    flow.strain_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_flow_strain: libf3d_host.so built against it must still load (RTLD_NOW) and solve, and
    flow_strain, OpticalFlow.strain and f3d_flow_strain_compute must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_flow_strain" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("extra,needle", [(["--strain", "vol,strain"], "usage"), (["--strain", ""], "usage"),
                                          (["--strain", "vol,,eq"], "usage"), (["--strain"], "usage"),
                                          (["--strain", "vol", "--partial"], "--strain"),
                                          (["--strain", "e,eq", "--concurrent", "2"], "--strain")])
def test_flow3d_strain_argument_errors(tmp_path, extra, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout
    assert not any("strain" in n or "flow-" in n for n in os.listdir(tmp_path))
