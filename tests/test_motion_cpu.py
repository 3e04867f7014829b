"""The motion fit without a GPU: f3d_motion_solve of the host library, fed with the sums of the numpy restatement
(tests/motion_ref.py), on displacements whose answer is known; the degenerate cases; the structs, the symbols of both headers, the weak
link of the host library and the argument errors of flow3d --detrend.

Bounds.  Affine: the sums of the dyadic constructions are exact, so the only error is the Cholesky solve of the 4 x 4 normal equations,
which is backward stable: 64 cond(N) 2^-53 max|coef| with cond(N) computed here from the normal matrix (a numpy prototype of the
solve showed at most 2.3e-16 against bounds of 4e-14 .. 1e-11).  Rigid: the polar rotation of B moves by at most 2 |dB| / (S2 + S3)
under a perturbation dB, and two correct decompositions of the same sums differ by a few rounding errors of size 2^-52 S1:
1e3 2^-52 S1 / (S2 + S3), with S from numpy's singular values."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import motion_ref as ref
from motion_ref import affine_field, holes, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SHAPES = [(7, 6, 5), (70, 24, 20), (130, 9, 33)]          # (W, H, D)
MODELS = {"translation": 0, "rigid": 1, "affine": 2}


def fill_sums(f3d, s):
    out = f3d.MotionSums()
    out.n = s["n"]
    for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
        getattr(out, name)[:] = s[name]
    return out


def solve(f3d, u, v, w, model, weight=None, weight_min=0.8):
    """f3d_motion_solve on the restatement's sums: (status, fit, message)"""
    d, h, w_ = u.shape
    sums = fill_sums(f3d, ref.motion_sums(u, v, w, weight, weight_min))
    fit = f3d.MotionFit()
    fit.centre[:] = [(w_ - 1) / 2, (h - 1) / 2, (d - 1) / 2]
    status = f3d.host().f3d_motion_solve(C.byref(sums), MODELS[model], C.byref(fit))
    return status, fit, f3d.host().f3d_host_last_error().decode()


# ---- affine recovery ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_holes", [False, True], ids=["full", "holes"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_recovers_dyadic_coefficients(f3d, dims, with_holes):
    w, h, d = dims
    rng = np.random.default_rng(w * 100 + h)
    M = rng.integers(-8, 9, (3, 3)) / 16.0                  # multiples of 1/16 within +-1/2
    t = rng.integers(-40, 41, 3) / 8.0                      # multiples of 1/8
    exact = affine_field((d, h, w), M, t)
    field = [a.astype(F32) for a in exact]
    for a, e in zip(field, exact):
        assert np.array_equal(a.astype(np.float64), e)      # every voxel value is a float32: the construction is exact
    if with_holes:
        for a in field:
            a[holes((d, h, w), 5)] = np.nan
    mask = ref.present_mask(*field)
    status, fit, msg = solve(f3d, *field, "affine")
    assert status == 0, msg
    _, _, N = ref.affine_lstsq(*field, mask)
    bound = 64 * np.linalg.cond(N) * 2.0 ** -53 * max(np.abs(M).max(), np.abs(t).max())
    err = max(np.abs(fit.matrix - M).max(), np.abs(np.array(list(fit.t)) - t).max())
    print(f"{dims} holes={with_holes}: error {err:.3g}, bound {bound:.3g}, cond {np.linalg.cond(N):.3g}")
    assert err <= bound, (err, bound)
    assert fit.n == int(mask.sum()) and fit.model == 2 and fit.cos_angle == 0 and list(fit.axial) == [0, 0, 0]
    rms = np.sqrt(sum(float((a[mask].astype(np.float64) ** 2).sum()) for a in field) / mask.sum())
    assert fit.rms_before == pytest.approx(rms, rel=1e-12)
    # translation on the same sums: the mean displacement, M = 0
    status, tr, msg = solve(f3d, *field, "translation")
    assert status == 0 and not np.any(tr.matrix)
    assert np.allclose(list(tr.t), [a[mask].astype(np.float64).mean() for a in field], rtol=1e-13, atol=1e-13)


# ---- rigid recovery ------------------------------------------------------------------------------------------------------------------------

def rigid_field(dims, noise=0.0, seed=1):
    w, h, d = dims
    R = rotation(0.05, (1, 2, 3))
    t = np.array([3.25, -1.5, 0.75])
    field = affine_field((d, h, w), R - np.eye(3), t)
    if noise:
        rng = np.random.default_rng(seed)
        field = [a + rng.normal(0, noise, a.shape) for a in field]
    return R, t, [a.astype(F32) for a in field]


@pytest.mark.parametrize("with_holes", [False, True], ids=["full", "holes"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rigid_agrees_with_numpy_kabsch(f3d, dims, with_holes):
    w, h, d = dims
    R_true, t_true, field = rigid_field(dims)
    if with_holes:
        for a in field:
            a[holes((d, h, w), 9)] = np.nan
    mask = ref.present_mask(*field)
    status, fit, msg = solve(f3d, *field, "rigid")
    assert status == 0, msg
    R = fit.matrix + np.eye(3)
    R_np, t_np, S = ref.kabsch(*field, mask)
    tol = 1e3 * 2.0 ** -52 * S[0] / (S[1] + S[2])
    err = np.abs(R - R_np).max()
    orth = np.abs(R.T @ R - np.eye(3)).sum(axis=1).max()
    print(f"{dims} holes={with_holes}: |R - R_numpy| {err:.3g} (tolerance {tol:.3g}), |R^T R - I| {orth:.3g}")
    assert err <= tol, (err, tol)
    assert orth <= 1e-14 and np.linalg.det(R) > 0
    assert np.abs(np.array(list(fit.t)) - t_np).max() <= tol * max(w, h, d)
    assert np.abs(R - R_true).max() < 1e-6 and np.abs(np.array(list(fit.t)) - t_true).max() < 1e-5    # float32 rounding of the data only
    assert fit.rms_before > 3
    assert fit.cos_angle == pytest.approx(np.cos(0.05), abs=1e-7)
    axial = np.array(list(fit.axial))
    assert np.allclose(axial, np.sin(0.05) * np.array([1, 2, 3]) / np.sqrt(14), atol=1e-7)
    assert fit.cos_angle == pytest.approx((np.trace(R) - 1) / 2, abs=1e-15)
    assert np.allclose(axial, [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2], rtol=0, atol=1e-16)


@pytest.mark.parametrize("dims", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_rigid_removal_leaves_the_noise(f3d, dims):
    """The rms of 3 n independent N(0, sigma^2) samples scatters by sigma sqrt 3 / sqrt(6 n) about sigma sqrt 3: 0.2 % for the two
    shapes here, far inside the 5 % asked for.  The 210 voxels of 7 x 6 x 5 would scatter by 2.8 %, so a 5 % test on them would fail
    by chance once in fourteen seeds; that shape is left to the tests above."""
    _, _, field = rigid_field(dims, noise=0.05, seed=dims[0])
    status, fit, msg = solve(f3d, *field, "rigid")
    assert status == 0, msg
    *_, stats = ref.remove_motion(*field, list(fit.centre), list(fit.t), list(fit.M))
    rms = np.sqrt(stats["sum_sq"] / stats["present"])
    print(f"{dims}: residual rms {rms:.4f} (sigma sqrt 3 = {0.05 * np.sqrt(3):.4f}), before {fit.rms_before:.4f}")
    assert abs(rms - 0.05 * np.sqrt(3)) <= 0.05 * 0.05 * np.sqrt(3)
    assert fit.rms_before > 3


# ---- degenerate cases ------------------------------------------------------------------------------------------------------------------------

def test_a_single_plane_has_no_z_column_but_a_rotation(f3d):
    w, h, d = 9, 7, 1
    R = rotation(0.03, (0, 0, 1))
    field = [a.astype(F32) for a in affine_field((d, h, w), R - np.eye(3), np.array([0.5, -0.25, 2.0]))]
    status, fit, msg = solve(f3d, *field, "affine")
    assert status == 0, msg
    assert not np.any(fit.matrix[:, 2]) and np.abs(fit.matrix[:, :2] - (R - np.eye(3))[:, :2]).max() < 1e-6
    status, fit, msg = solve(f3d, *field, "rigid")
    assert status == 0, msg
    Rg = fit.matrix + np.eye(3)
    assert np.abs(Rg - R).max() < 1e-6 and np.linalg.det(Rg) > 0 and np.abs(Rg.T @ Rg - np.eye(3)).max() <= 1e-14
    R_np, _, _ = ref.kabsch(*field, ref.present_mask(*field))
    assert np.abs(Rg - R_np).max() <= 1e-12


@pytest.mark.parametrize("dims", [(9, 1, 1), (1, 1, 12)], ids=["row", "column"])
def test_a_single_row_determines_a_translation_only(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(3)
    field = [rng.normal(1.0, 0.1, (d, h, w)).astype(F32) for _ in range(3)]
    for model, word in (("rigid", "collinear"), ("affine", "collinear")):
        status, _, msg = solve(f3d, *field, model)
        assert status != 0 and "f3d_motion_solve" in msg and word in msg, (model, msg)
    status, fit, msg = solve(f3d, *field, "translation")
    assert status == 0 and fit.n == w * h * d and not np.any(fit.matrix)


def test_no_present_voxel_is_refused_for_every_model(f3d):
    nan = np.full((3, 4, 5), np.nan, F32)
    for model in MODELS:
        status, fit, msg = solve(f3d, nan, nan, nan, model)
        assert status != 0 and "no voxel is present" in msg
        assert fit.n == 0 and not np.any(fit.matrix)                    # the fit is untouched
    zero = np.zeros((3, 4, 5), F32)
    status, _, msg = solve(f3d, zero, zero, zero, "rigid", weight=np.full((3, 4, 5), np.nan, F32))
    assert status != 0 and "no voxel is present" in msg
    sums = fill_sums(f3d, ref.motion_sums(zero, zero, zero))
    assert f3d.host().f3d_motion_solve(C.byref(sums), 3, C.byref(f3d.MotionFit())) != 0
    assert b"model" in f3d.host().f3d_host_last_error()
    assert f3d.host().f3d_motion_solve(None, 0, C.byref(f3d.MotionFit())) != 0


def test_a_coplanar_oblique_mask_refuses_the_affine_model(f3d):
    w, h, d = 7, 7, 5
    M = np.array([[0.25, 0, 0], [0, -0.125, 0], [0.0625, 0, 0.5]])
    field = [a.astype(F32) for a in affine_field((d, h, w), M, np.array([1.0, 2.0, 3.0]))]
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    weight = np.where(x + y == 6, 1.0, 0.0).astype(F32)                 # the plane x + y = 6: no axis is constant on it
    assert int((weight > 0).sum()) == 7 * 5
    status, _, msg = solve(f3d, *field, "affine", weight=weight, weight_min=0.5)
    assert status != 0 and "coplanar" in msg, msg
    status, fit, msg = solve(f3d, *field, "rigid", weight=weight, weight_min=0.5)   # a plane does determine a rotation
    assert status == 0 and fit.n == 35, msg
    status, fit, msg = solve(f3d, *field, "affine", weight=weight, weight_min=0.0)  # all voxels again
    assert status == 0 and np.abs(fit.matrix - M).max() < 1e-12


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------

def test_the_restatement_on_a_full_box_matches_the_closed_forms():
    for w, h, d in SHAPES:
        zero = np.zeros((d, h, w), F32)
        s = ref.motion_sums(zero, zero, zero)
        n = w * h * d
        assert s["n"] == n and s["x2"] == [0, 0, 0] and s["xx4"][3:] == [0, 0, 0]
        assert [4 * 3 * v for v in s["xx4"][:3]] == [4 * n * (w * w - 1), 4 * n * (h * h - 1), 4 * n * (d * d - 1)]   # sum X^2 = n (W^2 - 1) / 12
        assert s["Sxx"][0] == n * (w * w - 1) / 12


def test_the_restatement_removes_what_it_is_given():
    u, v, w = affine_field((4, 5, 6), np.diag([0.5, 0.25, 0.125]), np.array([1.0, 2.0, 3.0]), F32)
    u[1, 2, 3] = np.nan
    ru, rv, rw, st = ref.remove_motion(u, v, w, [2.5, 2.0, 1.5], [1.0, 2.0, 3.0], np.diag([0.5, 0.25, 0.125]))
    assert np.isnan(ru[1, 2, 3]) and rv[1, 2, 3] == 0 and st["present"] == 119 and st["sum_sq"] == 0 and st["max_abs"] == 0
    assert not np.any(np.nan_to_num(ru)) and not np.any(rv) and not np.any(rw)


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_the_header(f3d, tmp_path):
    """the header as C (where the struct and the entry f3d_motion_sums share a name) gives the sizes and offsets the binding uses"""
    src = tmp_path / "sizes.c"
    src.write_text(textwrap.dedent('''
        #include <stddef.h>
        #include <stdio.h>
        #include "f3d_host.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(struct f3d_motion_sums), offsetof(struct f3d_motion_sums, Sxd),
                 sizeof(f3d_motion_fit), offsetof(f3d_motion_fit, n), offsetof(f3d_motion_fit, axial), offsetof(f3d_motion_fit, model),
                 sizeof(f3d_motion_residual), offsetof(f3d_motion_residual, sum_sq), offsetof(f3d_motion_residual, max_abs));
          printf("%d %d %d\\n", F3D_MOTION_TRANSLATION, F3D_MOTION_RIGID, F3D_MOTION_AFFINE);
          return 0;
        }'''))
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [int(x) for x in lines[0].split()]
    S, Fit, Res = f3d.MotionSums, f3d.MotionFit, f3d.MotionResidual
    assert got == [C.sizeof(S), S.Sxd.offset, C.sizeof(Fit), Fit.n.offset, Fit.axial.offset, Fit.model.offset, C.sizeof(Res),
                   Res.sum_sq.offset, Res.max_abs.offset]
    assert got[0] == 200 and got[2] == 176 and got[6] == 24
    assert [int(x) for x in lines[1].split()] == [f3d.MOTION_MODELS[m] for m in ("translation", "rigid", "affine")]


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_motion_sums", "f3d_remove_motion"]),
                                              ("f3d_host.h", "host", ["f3d_motion_solve", "f3d_flow_motion_compute", "f3d_flow_motion_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    if header == "f3d.h":                                      # the definition stands in the header in full
        for needle in ("res_r = (float)((double)d_r - (t_r + ((M_r0 * X + M_r1 * Y) + M_r2 * Z)))", "X * s_j", "ascending z",
                       "weight[i] >= weight_min", "xx yy zz xy xz yz", "no float atomics"):
            assert needle in text, needle
    else:
        for needle in ("Kabsch", "Cholesky", "2^-40", "one-sidedly"):
            assert needle in text, needle


def test_the_binding_names(f3d):
    assert f3d.MOTION_MODELS == {"translation": 0, "rigid": 1, "affine": 2}
    sums_fn, remove_fn = f3d._motion_entry()
    assert len(sums_fn.argtypes) == 9 and sums_fn.argtypes[4] is C.c_float and len(remove_fn.argtypes) == 11
    for name in ("fit_motion", "remove_motion", "motion_sums", "solve_motion"):
        assert callable(getattr(f3d, name))
    assert hasattr(f3d.OpticalFlow, "motion") and hasattr(f3d.OpticalFlow, "motion_end")
    fit = f3d.MotionFit()
    fit.M[:] = range(9)
    assert fit.matrix.tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert set(fit.as_dict()) >= {"centre", "t", "matrix", "n", "rms_before"}
    with pytest.raises(ValueError):
        f3d._motion_model("similarity")


CASE = textwrap.dedent('''
    import ctypes as C, importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["F3D_ROOT"], "tests"))
    import motion_ref as ref
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    u, v, w = flow.download()
    # the solve is host code: it runs here, on the sums of the restatement
    s = ref.motion_sums(u, v, w)
    sums = pkg.MotionSums(); sums.n = s["n"]
    for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
        getattr(sums, name)[:] = s[name]
    fit = pkg.solve_motion(sums, (W, H, D), "rigid")
    assert fit.n == W * H * D and abs(fit.t[0] - u.mean()) < 1e-3
    for call in (lambda: flow.motion(), lambda: flow.motion(model="affine"), lambda: pkg.fit_motion(u, v, w),
                 lambda: pkg.motion_sums(u, v, w), lambda: pkg.remove_motion(u, v, w, fit)):
        try:
            call(); raise SystemExit("a call succeeded without f3d_motion_sums")
        except pkg.F3dError as e:
            assert "f3d_motion_sums" in str(e), str(e)
    flow.motion_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_and_solves_without_the_device_entries():
    """tests/cpu_device defines neither f3d_motion_sums nor f3d_remove_motion: libf3d_host.so built against it must still load
    (RTLD_NOW), solve flows and motion fits, and fit_motion, remove_motion and OpticalFlow.motion must fail with a message naming
    the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_motion_sums" not in names and "f3d_remove_motion" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("extra,needle", [(["--detrend", "similarity"], "usage"), (["--detrend", ""], "usage"), (["--detrend"], "usage"),
                                          (["--detrend", "rigid", "--detrend-min-zncc"], "usage"),
                                          (["--detrend", "rigid", "--detrend-min-zncc", "high"], "usage"),
                                          (["--detrend-min-zncc", "0.8", "--match", "zncc"], "--detrend-min-zncc needs --detrend"),
                                          (["--detrend", "rigid", "--detrend-min-zncc", "0.8"], "needs --match"),
                                          (["--detrend", "rigid", "--detrend-min-zncc", "0.8", "--match", "zncc", "--cumulative"],
                                           "--cumulative"),
                                          (["--detrend", "rigid", "--partial"], "--detrend"),
                                          (["--detrend", "affine", "--concurrent", "2"], "--detrend")])
def test_flow3d_detrend_argument_errors(tmp_path, extra, needle):
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
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--detrend translation|rigid|affine [--detrend-min-zncc T]]" in run.stdout
    assert "[--match warped,zncc,rmsd [--match-radius R]]" in run.stdout          # the earlier usage text is all still there
    assert not any("detrended" in n or "flow-" in n for n in os.listdir(tmp_path))
