"""Principal strains and the polar decomposition of a stored gradient without a GPU: the restatement (tests/from_gradient_ref.py, the
checker of f3d_principal_from_gradient and f3d_polar_from_gradient) against principal_ref and polar_ref on the central-difference
gradient, by bits; what the window's gradient buys on a noisy field (the bias of the eigenvalues of a noisy tensor); the binding's
argument checks; the host library's weak link to the two device entries; the argument errors of flow3d --window-principal and
--window-rotation; the symbols of both headers.

The bounds of the noise test are not taken from its results: 1 % and 10 % on the mean of gmax are the issue's, and the ratios of the
deviations are the textbook gains of f3d_window_strain's header (0.236, 0.063, 0.027 over 0.707 of the central difference) with a
margin of 1.25 for the quadratic term of E, which adds 6 % at radius 1.  MEASURED holds what this file measures."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from from_gradient_ref import (GRAD_NAMES, central_gradient, polar_from_gradient_ref, polar_stats, principal_from_gradient_ref,
                               principal_stats)
from polar_ref import NAMES as POLAR_NAMES, polar_ref, polar_stats_ref
from principal_ref import NAMES as PRINCIPAL_NAMES, principal_ref, principal_stats_ref
from strain_ref import same_bits
from window_strain_ref import window_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32


def rotation(angle, axis):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def noisy_field():
    """(u, v, w) float32 of shape (20, 22, 24): (F - I) (x, y, z), F = R U, U = diag(1.02, 0.99, 1.00), R 0.05 rad about
    (1, 2, 3) / sqrt(14), plus white noise of deviation 0.01 voxel from default_rng(5) drawn for u, then v, then w"""
    d, h, w = 20, 22, 24
    F = rotation(0.05, (1, 2, 3)) @ np.diag([1.02, 0.99, 1.00])
    z, y, x = np.meshgrid(np.arange(d, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    A = F - np.eye(3)
    rng = np.random.default_rng(5)
    return [(A[c, 0] * x + A[c, 1] * y + A[c, 2] * z + 0.01 * rng.standard_normal((d, h, w))).astype(F32) for c in range(3)]


def with_holes(rng, comps, share):
    out = [a.copy() for a in comps]
    for a in out:
        a[rng.random(a.shape) < share / 3] = np.nan
    return out


# ---- the restatement is the existing ones on the central-difference gradient ------------------------------------------------------------

@pytest.mark.parametrize("shape", [(20, 22, 24), (1, 7, 6), (5, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_the_central_gradient_gives_principal_ref_and_polar_ref_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape))
    comps = noisy_field() if shape == (20, 22, 24) else [rng.uniform(-0.3, 0.3, size=shape).astype(F32) for _ in range(3)]
    comps = with_holes(rng, comps, 0.25)
    grad = central_gradient(*comps)
    undefined = np.isnan(grad[0])
    assert all(np.array_equal(np.isnan(g), undefined) for g in grad)
    if comps[0].size > 100:
        assert 0.2 < undefined.mean() < 0.9

    want = principal_ref(*comps)
    got = principal_from_gradient_ref(grad)
    for n in PRINCIPAL_NAMES:
        assert same_bits(got[n], want[n]), n
    assert principal_stats(got) == principal_stats_ref(want["e1"], want["e3"], want["gmax"]) or not (~undefined).any()

    want, want_folded = polar_ref(*comps)
    got, folded = polar_from_gradient_ref(grad)
    for n in POLAR_NAMES:
        assert same_bits(got[n], want[n]), n
    assert np.array_equal(folded, want_folded)
    a, b = polar_stats(got, folded), polar_stats_ref(want, want_folded)
    assert all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in b), (a, b)


def test_any_nan_entry_makes_the_voxel_undefined_and_nothing_else_does():
    rng = np.random.default_rng(3)
    grad = [rng.normal(0, 0.05, size=(4, 5, 27)).astype(F32) for _ in range(9)]
    for k in range(9):
        grad[k][:, :, 3 * k] = np.nan            # one entry each
    grad[4][0, 0, 1] = np.inf                    # not a NaN: the arithmetic runs
    bad = np.zeros((4, 5, 27), bool)
    bad[:, :, 0:27:3] = True
    p = principal_from_gradient_ref(grad)
    q, folded = polar_from_gradient_ref(grad)
    for n in PRINCIPAL_NAMES:
        assert np.isnan(p[n][bad]).all(), n
    for n in ("e1", "e2", "e3", "gmax"):
        good = ~bad
        good[0, 0, 1] = False
        assert not np.isnan(p[n][good]).any(), n
    for n in POLAR_NAMES:
        assert np.isnan(q[n][bad]).all() and not folded[bad].any(), n
    st = polar_stats(q, folded)
    assert st["defined"] + st["folded"] == int((~bad).sum())
    assert principal_stats(p)["defined"] == int((~np.isnan(p["e1"])).sum())


# ---- what the window's gradient buys ------------------------------------------------------------------------------------------------------

TRUE_GMAX, TRUE_E1 = 0.5 * (0.5 * (1.02 ** 2 - 1) - 0.5 * (0.99 ** 2 - 1)), 0.5 * (1.02 ** 2 - 1)      # 0.015075, 0.0202
GAIN = {1: 0.236 / 0.707, 2: 0.063 / 0.707, 3: 0.027 / 0.707}                                          # 0.334, 0.089, 0.038
# gradient -> (mean gmax, std e1, rms error of theta) over the interior [4:-4]^3, measured by the test below
MEASURED = {
    "central": (0.018038, 0.006880, 0.004980),    # +19.66 %
    1: (0.015378, 0.002441, 0.001654),            # +2.01 %, deviation x 0.355
    2: (0.015085, 0.000623, 0.000437),            # +0.06 %, x 0.091
    3: (0.015068, 0.000264, 0.000189),            # -0.04 %, x 0.038
}


def test_the_window_gradient_removes_the_bias_of_noisy_eigenvalues(capsys):
    comps = noisy_field()
    inner = (slice(4, -4),) * 3

    def figures(grad):
        p = principal_from_gradient_ref(grad)
        q, _ = polar_from_gradient_ref(grad)
        g, e1, th = (a[inner].astype(np.float64) for a in (p["gmax"], p["e1"], q["theta"]))
        assert not (np.isnan(g).any() or np.isnan(th).any())
        return float(g.mean()), float(e1.std()), float(np.sqrt(np.mean((th - 0.05) ** 2)))

    got = {"central": figures(central_gradient(*comps))}
    for r in (1, 2, 3):
        G, _, fitted = window_gradient(*comps, r)
        got[r] = figures([np.where(fitted, G[c][a], F32(np.nan)).astype(F32) for c in range(3) for a in range(3)])
    with capsys.disabled():
        for k, (g, s, t) in got.items():
            print(f"\n  gradient {k}: mean gmax {g:.6f} ({100 * (g / TRUE_GMAX - 1):+.2f} %), std e1 {s:.6f} "
                  f"(x {s / got['central'][1]:.3f}), rms error of theta {t:.6f}", end="")
        print()

    assert abs(TRUE_GMAX - 0.015075) < 1e-9 and abs(TRUE_E1 - 0.0202) < 1e-9
    assert got["central"][0] / TRUE_GMAX - 1 > 0.10
    for r in (2, 3):
        assert abs(got[r][0] / TRUE_GMAX - 1) < 0.01, (r, got[r][0])
    for r in (1, 2, 3):
        ratio = got[r][1] / got["central"][1]
        assert GAIN[r] / 1.25 <= ratio <= GAIN[r] * 1.25, (r, ratio, GAIN[r])
        assert got[r][2] < got["central"][2]
    for k in got:                                     # the table in DESIGN.md section 21 is this one
        assert got[k] == pytest.approx(MEASURED[k], rel=5e-3), (k, got[k])


# ---- the binding's argument checks (nothing here reaches a device) -----------------------------------------------------------------------

def test_the_binding_checks_its_arguments_before_the_device(f3d):
    a = np.zeros((3, 4, 5), np.float32)
    nine = [a] * 9
    for bad in ([a] * 8, [a] * 10, [a] * 8 + [np.zeros((3, 4, 6), np.float32)], [a] * 8 + [np.zeros((4, 5), np.float32)], [], None, 3,
                {n: a for n in GRAD_NAMES[:8]}):
        for fn in (f3d.principal_from_gradient, f3d.polar_from_gradient):
            with pytest.raises(ValueError):
                fn(bad)
    for fields in ("", "val,", "angle", ("val", "axis"), ()):
        with pytest.raises(ValueError):
            f3d.principal_from_gradient(nine, fields=fields)
        with pytest.raises(ValueError):
            f3d.window_principal(a, a, a, fields=fields)
    for fields in ("", "angle,", "val", ("angle", "axis"), ()):
        with pytest.raises(ValueError):
            f3d.polar_from_gradient(nine, fields=fields)
        with pytest.raises(ValueError):
            f3d.window_rotation(a, a, a, fields=fields)
    for fn, method in ((f3d.window_principal, f3d.OpticalFlow.window_principal), (f3d.window_rotation, f3d.OpticalFlow.window_rotation)):
        for kw in (dict(radius=0), dict(radius=4), dict(radius=1.5), dict(radius=1, min_count=28), dict(radius=2, min_count=0),
                   dict(radius=3, min_count=344), dict(radius=2, min_count=2.5)):
            with pytest.raises(ValueError):
                fn(a, a, a, **kw)
            with pytest.raises(ValueError):
                method(None, **kw)                   # the checks come before the driver is looked at
        with pytest.raises(ValueError):
            method(None, source="pair")
        with pytest.raises(ValueError):
            fn(a, a, np.zeros((3, 4, 6), np.float32))
    assert f3d._window_args(1, None) == (1, 6) and f3d._window_args(2, None) == (2, 31) and f3d._window_args(3, 343) == (3, 343)
    assert f3d.GRADIENT_NAMES == GRAD_NAMES == f3d.WINDOW_STRAIN_NAMES[8:]
    for name in ("_principal_from_gradient_entry", "_polar_from_gradient_entry"):
        assert callable(getattr(f3d, name))
    for name in ("window_principal", "window_principal_end", "window_rotation", "window_rotation_end"):
        assert callable(getattr(f3d.OpticalFlow, name))


# ---- the weak link of the host library ---------------------------------------------------------------------------------------------

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
    grad = [u] * 9
    for entry, calls in (("f3d_principal_from_gradient", (lambda: flow.window_principal("flow"), lambda: flow.window_principal(fields="dir1"),
                                                          lambda: pkg.principal_from_gradient(grad), lambda: pkg.window_principal(u, v, w))),
                         ("f3d_polar_from_gradient", (lambda: flow.window_rotation("flow"), lambda: flow.window_rotation(fields="stretch"),
                                                      lambda: pkg.polar_from_gradient(grad), lambda: pkg.window_rotation(u, v, w)))):
        for call in calls:
            try:
                call(); raise SystemExit("a call succeeded without " + entry)
            except pkg.F3dError as e:
                assert entry in str(e), str(e)
    # the C API itself, without the binding in between
    host = pkg.host()
    ptrs = (pkg._fp * 10)(*[np.empty((D, H, W), np.float32).ctypes.data_as(pkg._fp) for _ in range(10)])
    assert host.f3d_flow_window_principal_compute(flow._h, 0, 15, 2, 31, ptrs, None) != 0
    assert b"f3d_principal_from_gradient" in host.f3d_host_last_error()
    assert host.f3d_flow_window_polar_compute(flow._h, 0, 7, 2, 31, ptrs, None) != 0
    assert b"f3d_polar_from_gradient" in host.f3d_host_last_error()
    try:
        flow.window_rotation("trajectory"); raise SystemExit("the window rotation of a trajectory that was never started succeeded")
    except pkg.F3dError as e:
        assert "trajectory" in str(e), str(e)
    flow.window_principal_end(); flow.window_rotation_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_principal_from_gradient nor f3d_polar_from_gradient: libf3d_host.so built against it must
    still load (RTLD_NOW) and solve, and every call that needs one of them must fail with a message naming it"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "from_gradient" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- flow3d --window-principal / --window-rotation -------------------------------------------------------------------------------------

def run_flow3d(tmp_path, extra):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    return subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,needle", [
    (["--window-principal", "val,axis"], "usage"), (["--window-principal", ""], "usage"), (["--window-principal", "val,,shear"], "usage"),
    (["--window-principal"], "usage"), (["--window-principal", "angle"], "usage"),
    (["--window-rotation", "angle,axis"], "usage"), (["--window-rotation", ""], "usage"), (["--window-rotation", "angle,,stretch"], "usage"),
    (["--window-rotation"], "usage"), (["--window-rotation", "val"], "usage"),
    (["--window-principal", "val", "--partial"], "--window-principal"), (["--window-principal", "dir1", "--concurrent", "2"], "--window-principal"),
    (["--window-rotation", "angle", "--partial"], "--window-rotation"), (["--window-rotation", "stretch", "--concurrent", "2"], "--window-rotation"),
    (["--window-radius", "2"], "--window-radius"), (["--window-min-count", "9"], "--window-radius"),
    (["--principal", "val", "--window-radius", "2"], "--window-radius"), (["--rotation", "angle", "--window-min-count", "5"], "--window-radius"),
    (["--window-principal", "val", "--window-radius", "4"], "usage"), (["--window-rotation", "angle", "--window-radius", "0"], "usage"),
    (["--window-principal", "val", "--window-radius", "1", "--window-min-count", "28"], "--window-min-count"),
    (["--window-rotation", "angle", "--window-radius", "1", "--window-min-count", "28"], "--window-min-count")])
def test_flow3d_argument_errors(tmp_path, extra, needle):
    run = run_flow3d(tmp_path, extra)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "--window-principal val,shear,dir1,dir3" in run.stdout and "--window-rotation angle,vector,stretch" in run.stdout
    assert "Allocating" not in run.stdout               # no device was touched
    assert not any("wprincipal" in n or "wrotation" in n or "flow-" in n for n in os.listdir(tmp_path))


@pytest.mark.parametrize("extra", [["--window-principal", "val", "--window-radius", "1"], ["--window-rotation", "angle", "--window-min-count", "9"],
                                   ["--window-principal", "val,shear,dir1,dir3", "--window-rotation", "angle,vector,stretch",
                                    "--window-radius", "3", "--window-min-count", "343"]])
def test_flow3d_accepts_the_window_options_with_either_new_option(tmp_path, extra):
    """the other direction of the rule: these pass the argument checks, so whatever happens next (there may be no device) is not the
    usage and not exit 64"""
    run = run_flow3d(tmp_path, extra)
    assert run.returncode != 64 and "usage" not in run.stdout, (run.returncode, run.stdout[-1000:])


# ---- the headers -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("header,lib,names", [
    ("f3d.h", "hip", ["f3d_principal_from_gradient", "f3d_polar_from_gradient"]),
    ("f3d_host.h", "host", ["f3d_flow_window_principal_compute", "f3d_flow_window_principal_end", "f3d_flow_window_polar_compute",
                            "f3d_flow_window_polar_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    assert not [n for n in have if not hasattr(handle, n)]
