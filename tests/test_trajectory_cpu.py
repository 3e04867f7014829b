"""Trajectory accumulation without a GPU: the float32 restatement of the composition step (tests/trajectory_ref.py, the checker of
f3d_compose_flow) against a float64 trilinear reference and on its edge cases, and the host library's weak link to the device
entry: built against a device library that lacks f3d_compose_flow it still loads and solves, and the trajectory calls fail with
a message naming the entry."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from trajectory_ref import compose_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")


def trilinear64(f, xf, yf, zf):
    """textbook trilinear interpolation in float64 at in-volume points"""
    f = f.astype(np.float64)
    d, h, w = f.shape
    x0, y0, z0 = (np.floor(t).astype(np.int64) for t in (xf, yf, zf))
    tx, ty, tz = xf - x0, yf - y0, zf - z0
    x1, y1, z1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1), np.minimum(z0 + 1, d - 1)
    out = np.zeros_like(xf)
    for zz, wz in ((z0, 1 - tz), (z1, tz)):
        for yy, wy in ((y0, 1 - ty), (y1, ty)):
            for xx, wx in ((x0, 1 - tx), (x1, tx)):
                out += wz * wy * wx * f[zz, yy, xx]
    return out


@pytest.mark.parametrize("shape", [(11, 23, 37), (5, 9, 64), (1, 1, 1)])
def test_restatement_agrees_with_float64_trilinear_inside(shape):
    rng = np.random.default_rng(sum(shape))
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    # targets strictly inside, as positions the float32 add reproduces
    tgt = [rng.uniform(0, n - 1, size=shape).astype(np.float32) for n in (w, h, d)]
    acc = tuple((t - c.astype(np.float32)).astype(np.float32) for t, c in zip(tgt, (x, y, z)))
    inc = tuple(rng.uniform(-3, 3, size=shape).astype(np.float32) for _ in range(3))
    got = compose_ref(acc, inc)
    pos = [(c.astype(np.float32) + a).astype(np.float64) for c, a in zip((x, y, z), acc)]
    for g, a, f in zip(got, acc, inc):
        want = a.astype(np.float64) + trilinear64(f, *pos)
        assert not np.isnan(g).any()
        assert np.allclose(g, want, rtol=0, atol=1e-5 * (1 + np.abs(want).max()))


def test_from_zero_the_step_gives_the_flow_exactly():
    rng = np.random.default_rng(1)
    shape = (6, 7, 9)
    inc = [rng.uniform(-2, 2, size=shape).astype(np.float32) for _ in range(3)]
    inc[0][0, 0, :3] = -0.0
    got = compose_ref(tuple(np.zeros(shape, np.float32) for _ in range(3)), inc)
    for g, f in zip(got, inc):
        assert np.array_equal(g, f)
        assert not np.signbit(g[f == 0]).any()      # -0 comes back as +0


def test_points_that_leave_become_nan_in_all_components_and_stay_nan():
    shape = (5, 6, 7)
    d, h, w = shape
    acc = [np.zeros(shape, np.float32) for _ in range(3)]
    inc = [np.full(shape, 0.25, np.float32) for _ in range(3)]
    # one voxel out through every face, one with NaN in one component, one that is infinite
    acc[0][2, 3, 0] = -0.5
    acc[0][2, 3, w - 1] = 0.5
    acc[1][1, 0, 2] = -1.0
    acc[1][1, h - 1, 2] = 3.0
    acc[2][0, 2, 2] = -0.01
    acc[2][d - 1, 2, 3] = 0.01
    acc[1][3, 3, 3] = np.nan
    acc[2][3, 4, 4] = np.inf
    out = [(2, 3, 0), (2, 3, w - 1), (1, 0, 2), (1, h - 1, 2), (0, 2, 2), (d - 1, 2, 3), (3, 3, 3), (3, 4, 4)]
    got = compose_ref(acc, inc)
    want_nan = np.zeros(shape, bool)
    for p in out:
        want_nan[p] = True
    for g in got:
        assert np.array_equal(np.isnan(g), want_nan)
    # a lost point stays lost whatever the next flow says (one that would bring it back inside included)
    back = [np.full(shape, -0.25, np.float32)] * 3
    again = compose_ref(got, back)
    for g in again:
        assert np.isnan(g)[want_nan].all()
        # (the rest moved by 0.25 in the first step: the far faces are outside now, everything else inside)
        assert not np.isnan(g)[:d - 1, :h - 1, :w - 1][~want_nan[:d - 1, :h - 1, :w - 1]].any()


def test_the_faces_themselves_are_inside():
    shape = (4, 5, 6)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    inc = [np.full(shape, 1.5, np.float32) for _ in range(3)]
    # every point to x_f = W-1, y_f = 0, z_f = D-1 exactly
    acc = [(w - 1 - x).astype(np.float32), (-y).astype(np.float32), (d - 1 - z).astype(np.float32)]
    got = compose_ref(acc, inc)
    for g, a in zip(got, acc):
        assert not np.isnan(g).any() and np.array_equal(g, a + np.float32(1.5))
    # one ulp further out is outside: x_f just above W-1 (column x = 0), y_f just below 0 (row y = 0 of column x = 1)
    acc[0][:, :, 0] = np.nextafter(np.float32(w - 1), np.float32(np.inf))
    acc[1][:, 0, 1] = np.nextafter(np.float32(0), np.float32(-np.inf))
    got = compose_ref(acc, inc)
    lost = np.zeros(shape, bool)
    lost[:, :, 0] = True
    lost[:, 0, 1] = True
    for g in got:
        assert np.array_equal(np.isnan(g), lost)


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
    u, v, w = flow.compute(f0, f1, silent=True, **kw)
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))
    for call in (flow.trajectory_begin, lambda: pkg.compose_flow((u, v, w), (u, v, w))):
        try:
            call(); raise SystemExit("a trajectory call succeeded without f3d_compose_flow")
        except pkg.F3dError as e:
            assert "f3d_compose_flow" in str(e), str(e)
    try:
        flow.trajectory_append(); raise SystemExit("append before begin succeeded")
    except pkg.F3dError as e:
        assert "begin" in str(e), str(e)
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_compose_flow: libf3d_host.so built against it must still load (RTLD_NOW) and solve,
    and every trajectory call must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_compose_flow" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
