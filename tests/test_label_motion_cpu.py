"""The per-label motion without a GPU: the numpy restatement (tests/label_motion_ref.py) against a brute-force loop, f3d_motion_solve_labels
of the host library against f3d_motion_solve fed each label's sums, dyadic affine maps per label, the argument checks of the binding,
the weak link of the host library and the argument errors of flow3d --labels / --label-motion.

Bounds.  Recentring: for the rigid model f3d_motion_solve gives t = dbar - s with s = (M xbar) in a stated order, and
f3d_motion_solve_labels adds the same s back, so t differs from dbar = Sd / n by the roundings of one subtraction and one addition of
numbers no larger than max(|dbar|, |s|): 64 2^-53 max|coef| with coef the numbers that enter (dbar, s, t about the volume centre).
Dyadic affine maps: M in sixteenths, t in eighths and half-integer coordinates make every displacement a multiple of 2^-5 below 1024,
so the quantisation to 2^-14 is exact (asserted) and the sums are those of tests/test_motion_cpu.py, whose bound
64 cond(N) 2^-53 max|coef| of the Cholesky solve holds for M; the recentred t = t_c + M xbar carries the error of t_c plus three
entries of M times |xbar_a| and a few roundings of its own size: bound (1 + 3 max|xbar|) + 8 2^-53 max|t|."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import label_motion_ref as ref
import motion_ref
from motion_ref import affine_field, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
MODELS = {"translation": 0, "rigid": 1, "affine": 2}


def fill_sums(f3d, per_label):
    out = (f3d.MotionSums * len(per_label))()
    for s, e in zip(out, per_label):
        s.n = e["n"]
        for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
            getattr(s, name)[:] = e[name]
    return out


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------

def test_the_restatement_against_a_loop_per_label():
    w, h, d = 7, 6, 5
    rng = np.random.default_rng(1)
    u, v, ww = (rng.uniform(-1100, 1100, (d, h, w)).astype(F32) for _ in range(3))
    u[0, 0, 0] = np.nan
    v[1, 2, 3] = np.inf
    ww[2, 2, 2] = F32(1024)
    u[3, 3, 3] = F32(2.5 / 16384)                            # a tie: to the even 2
    u[3, 3, 4] = F32(-3.5 / 16384)                           # to the even -4
    weight = rng.choice(np.array([0.5, 0.8, 1.0, np.nan], F32), size=(d, h, w))
    labels = rng.integers(-1, 5, (d, h, w)).astype(np.int32)  # -1 and 4 are foreign with n_labels = 3
    got, info = ref.label_integers(u, v, ww, labels, 3, weight, 0.8)
    want = [{"n": 0, "x2": [0] * 3, "xx4": [0] * 6, "Id": [0] * 3, "Ixd": [0] * 9, "Idd": [0] * 3} for _ in range(3)]
    counts = dict.fromkeys(ref.INFO, 0)
    for z in range(d):
        for y in range(h):
            for x in range(w):
                L = int(labels[z, y, x])
                dd = [u[z, y, x], v[z, y, x], ww[z, y, x]]
                if L == 0:
                    counts["background"] += 1
                elif L < 0 or L > 3:
                    counts["foreign"] += 1
                elif any(np.isnan(c) for c in dd) or not weight[z, y, x] >= F32(0.8):
                    counts["absent"] += 1
                elif any(abs(c) >= 1024 for c in dd):
                    counts["out_of_range"] += 1
                else:
                    counts["used"] += 1
                    s = want[L - 1]
                    c2 = [2 * x - (w - 1), 2 * y - (h - 1), 2 * z - (d - 1)]
                    q = []
                    for c in dd:
                        scaled = float(c) * 16384.0              # exact in binary64 too
                        r = int(np.floor(scaled))
                        frac = scaled - r
                        q.append(r + (1 if frac > 0.5 or (frac == 0.5 and r % 2) else 0))
                    s["n"] += 1
                    for i in range(3):
                        s["x2"][i] += c2[i]
                        s["Id"][i] += q[i]
                        s["Idd"][i] += q[i] * q[i]
                        for j in range(3):
                            s["Ixd"][3 * i + j] += c2[i] * q[j]
                    for m, (i, k) in enumerate(motion_ref.SXX_ORDER):
                        s["xx4"][m] += c2[i] * c2[k]
    assert info == counts and all(v > 0 for v in counts.values())
    assert got == want
    assert ref.quantise(np.array([2.5 / 16384, -3.5 / 16384, 0.5 / 16384, 1.5 / 16384], F32)).tolist() == [2, -4, 0, 2]
    sums, _ = ref.label_sums(u, v, ww, labels, 3, weight, 0.8)
    for s, e in zip(sums, want):
        assert s["Sd"] == [i / 16384 for i in e["Id"]] and s["Sxd"] == [i / 32768 for i in e["Ixd"]]   # small integers: exact
        assert s["Sx"] == [i / 2 for i in e["x2"]] and s["Sxx"] == [i / 4 for i in e["xx4"]]
    assert ref.scaled(2 ** 80 + 2 ** 27, -28) == 2.0 ** 52 and ref.scaled(2 ** 80 + 3 * 2 ** 27, -28) == 2.0 ** 52 + 2.0   # ties to even, once


def test_the_restatement_removes_what_it_is_given():
    shape = (4, 5, 6)
    labels = np.ones(shape, np.int32)
    labels[:, :, 3:] = 2
    labels[0, 0, 0] = 0
    labels[0, 0, 5] = 7
    M1, t1 = np.diag([0.5, 0.25, 0.125]), np.array([1.0, 2.0, 3.0])
    u, v, w = affine_field(shape, M1, t1, F32)
    centre = [[2.5, 2.0, 1.5], [2.5, 2.0, 1.5], [0, 0, 0]]
    ru, rv, rw, st = ref.remove_label_motion(u, v, w, labels, centre, [t1, t1 + 1, t1], [M1, M1, M1], [True, True, False])
    assert np.isnan(ru[0, 0, 0]) and np.isnan(rw[0, 0, 5]) and st["present"] == 118
    one, two = labels == 1, (labels == 2)
    assert not ru[one].any() and not rv[one].any() and (ru[two] == -1).all() and (rw[two] == -1).all() and st["max_abs"] == 1


# ---- f3d_motion_solve_labels -------------------------------------------------------------------------------------------------------------------

def cell_case(dims, seeds, model_noise=0.01):
    w, h, d = dims
    labels = ref.voronoi((d, h, w), seeds, seed=4)
    rng = np.random.default_rng(8)
    field = [np.zeros((d, h, w)) for _ in range(3)]
    for L in range(1, seeds + 1):
        whole = affine_field((d, h, w), rotation(rng.uniform(-0.1, 0.1), rng.normal(size=3)) - np.eye(3), rng.uniform(-5, 5, 3))
        for a, b in zip(field, whole):
            a[labels == L] = b[labels == L]
    field = [(a + rng.normal(0, model_noise, a.shape)).astype(F32) for a in field]
    return labels, field


@pytest.mark.parametrize("model", list(MODELS))
def test_solve_labels_is_solve_per_label_moved_to_the_centroid(f3d, model):
    dims = (30, 20, 16)
    w, h, d = dims
    labels, field = cell_case(dims, 9)
    labels[labels == 3] = 0                                   # empty
    labels[0, 0, :] = 0
    labels[0, 0, 2:12] = 10                                   # ten voxels in a row: small at 27, degenerate (collinear) at 5
    labels[1, 0:3, 0:3] = 11                                  # nine voxels of a plane z = 1
    n_labels = 12                                             # label 12 does not occur
    per_label, info = ref.label_sums(*field, labels, n_labels)
    sums = fill_sums(f3d, per_label)
    centre = [(w - 1) / 2, (h - 1) / 2, (d - 1) / 2]
    for min_voxels, small in ((27, {10, 11}), (5, set())):
        motion = f3d.solve_label_motion(sums, dims, model, min_voxels)
        assert motion.n.tolist() == [s["n"] for s in per_label]
        for L in range(1, n_labels + 1):
            i = L - 1
            one = f3d.MotionFit()
            status = f3d.host().f3d_motion_solve(C.byref(sums[i]), MODELS[model], C.byref(one))
            if per_label[i]["n"] == 0:
                want = ref.EMPTY
            elif L in small:
                want = ref.SMALL
            else:
                want = ref.OK if status == 0 else ref.DEGENERATE
            assert motion.status[i] == want, (L, model, min_voxels)
            if want != ref.OK:
                assert not motion.t[i].any() and not motion.matrix[i].any() and not motion.centre[i].any() and motion.rms_before[i] == 0
                continue
            # the recentring identity, in the header's order, exactly
            c, t = ref.recentre(per_label[i], centre, list(one.t), list(one.M))
            assert motion.centre[i].tolist() == c and motion.t[i].tolist() == t
            assert motion.matrix[i].tolist() == one.matrix.tolist() and motion.rms_before[i] == one.rms_before
            assert motion.cos_angle[i] == one.cos_angle and motion.axial[i].tolist() == list(one.axial)
            n = per_label[i]["n"]
            xbar = np.array(per_label[i]["Sx"]) / n
            assert np.allclose(motion.centre[i], [np.argwhere(labels == L)[:, k].mean() for k in (2, 1, 0)], rtol=0, atol=1e-9)
            if model != "affine":
                # t at the centroid is the mean displacement of the body (translation: M = 0; rigid: dbar - M xbar + M xbar)
                dbar = np.array(per_label[i]["Sd"]) / n
                s = one.matrix @ xbar
                coef = max(np.abs(dbar).max(), np.abs(s).max(), np.abs(np.array(list(one.t))).max())
                assert np.abs(motion.t[i] - dbar).max() <= 64 * 2.0 ** -53 * coef, (L, motion.t[i], dbar)
        if min_voxels == 5:
            expect = {"translation": ref.OK, "rigid": ref.DEGENERATE, "affine": ref.DEGENERATE}[model]
            assert motion.status[9] == expect                 # a row of voxels determines a translation only
            assert motion.status[10] == ref.OK                # a plane determines all three (the affine map with a zero column)
        assert motion.status[2] == ref.EMPTY and motion.status[11] == ref.EMPTY
    assert f3d.LABEL_STATUS == ("ok", "empty", "small", "degenerate")


def test_solve_labels_refusals(f3d):
    host = f3d.host()
    sums = (f3d.MotionSums * 2)()
    fits, status = (f3d.MotionFit * 2)(), (C.c_int * 2)(7, 7)
    centre = (C.c_double * 3)(1, 1, 1)
    assert host.f3d_motion_solve_labels(sums, 2, 3, 27, centre, fits, status) != 0 and b"model" in host.f3d_host_last_error()
    assert host.f3d_motion_solve_labels(sums, 2, -1, 27, centre, fits, status) != 0
    for args in ((None, 2, 1, 27, centre, fits, status), (sums, 2, 1, 27, None, fits, status), (sums, 2, 1, 27, centre, None, status),
                 (sums, 2, 1, 27, centre, fits, None)):
        assert host.f3d_motion_solve_labels(*args) != 0 and b"f3d_motion_solve_labels" in host.f3d_host_last_error()
    assert list(status) == [7, 7]                              # nothing written
    assert host.f3d_motion_solve_labels(sums, 2, 1, 27, centre, fits, status) == 0 and list(status) == [ref.EMPTY, ref.EMPTY]
    assert host.f3d_motion_solve_labels(sums, 0, 1, 27, centre, fits, status) == 0     # no label: nothing to do
    with pytest.raises(ValueError):
        f3d.solve_label_motion(sums, (4, 4, 4), "similarity")


@pytest.mark.parametrize("dims", [(7, 6, 5), (70, 24, 20), (130, 9, 33)], ids=lambda s: "x".join(map(str, s)))
def test_every_label_recovers_its_own_dyadic_affine_map(f3d, dims):
    w, h, d = dims
    seeds = 2 if w < 10 else 6
    rng = np.random.default_rng(w * 100 + h)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    labels = (1 + (x * seeds) // w).astype(np.int32)          # slabs along x: every body spans y and z and several x
    labels[(y == 0) & (z == 0)] = 0
    maps = [(rng.integers(-8, 9, (3, 3)) / 16.0, rng.integers(-40, 41, 3) / 8.0) for _ in range(seeds)]
    field = [np.zeros((d, h, w)) for _ in range(3)]
    for L, (M, t) in enumerate(maps, 1):
        for a, b in zip(field, affine_field((d, h, w), M, t)):
            a[labels == L] = b[labels == L]
    f32 = [a.astype(F32) for a in field]
    for a, e in zip(f32, field):
        assert np.array_equal(a.astype(np.float64), e) and np.abs(e).max() < 1024
        assert np.array_equal(ref.quantise(a).astype(np.float64) * 2.0 ** -14, e)       # the quantisation is exact
    per_label, info = ref.label_sums(*f32, labels, seeds)
    assert info["used"] == int((labels > 0).sum()) and info["background"] == w
    motion = f3d.solve_label_motion(fill_sums(f3d, per_label), dims, "affine", 27 if w > 10 else 8)
    assert (motion.status == ref.OK).all()
    for L, (M, t) in enumerate(maps, 1):
        i = L - 1
        mask = labels == L
        _, _, N = motion_ref.affine_lstsq(*f32, mask)
        bound = 64 * np.linalg.cond(N) * 2.0 ** -53 * max(np.abs(M).max(), np.abs(t).max())
        xbar = np.array(per_label[i]["Sx"]) / per_label[i]["n"]
        t_here = t + M @ xbar
        err_M = np.abs(motion.matrix[i] - M).max()
        err_t = np.abs(motion.t[i] - t_here).max()
        bound_t = bound * (1 + 3 * np.abs(xbar).max()) + 8 * 2.0 ** -53 * max(np.abs(t_here).max(), np.abs(t).max())
        print(f"{dims} label {L}: |dM| {err_M:.3g} (bound {bound:.3g}), |dt| {err_t:.3g} (bound {bound_t:.3g})")
        assert err_M <= bound and err_t <= bound_t
        assert motion.n[i] == int(mask.sum())


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_the_header(f3d, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(textwrap.dedent('''
        #include <stddef.h>
        #include <stdio.h>
        #include "f3d_host.h"
        int main(void) {
          printf("%zu %zu %zu\\n", sizeof(f3d_label_info), offsetof(f3d_label_info, out_of_range), offsetof(f3d_label_info, used));
          printf("%d %d %d %d\\n", F3D_LABEL_OK, F3D_LABEL_EMPTY, F3D_LABEL_SMALL, F3D_LABEL_DEGENERATE);
          return 0;
        }'''))
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    I = f3d.LabelInfo
    assert [int(x) for x in lines[0].split()] == [C.sizeof(I), I.out_of_range.offset, I.used.offset] == [40, 24, 32]
    assert [int(x) for x in lines[1].split()] == [ref.OK, ref.EMPTY, ref.SMALL, ref.DEGENERATE] == [0, 1, 2, 3]


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_label_motion_sums", "f3d_remove_label_motion"]),
                                              ("f3d_host.h", "host", ["f3d_motion_solve_labels", "f3d_flow_label_motion_compute",
                                                                      "f3d_flow_label_motion_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    if header == "f3d.h":                                      # the definition stands in the header in full
        for needle in ("q_j = (int)rintf(d_j * 16384.0f)", "ties to even", "v & 0xffffffff", "v >> 32", "2^-14 Id_j", "2^-15 Ixd_ij",
                       "2^-28 Idd_j", "|d_j| < 1024", "out_of_range", "Idd reaches 2^81", "1 .. 2^22"):
            assert needle in text, needle
    else:
        for needle in ("centre_a = volume_centre_a + xbar_a", "t_r + ((M_r0 * xbar_0 + M_r1 * xbar_1) + M_r2 * xbar_2)",
                       "F3D_LABEL_DEGENERATE"):
            assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    sums_fn, remove_fn = f3d._label_motion_entry()
    assert len(sums_fn.argtypes) == 12 and sums_fn.argtypes[6] is C.c_float and len(remove_fn.argtypes) == 14
    zero = np.zeros((3, 4, 5), F32)
    good = np.ones((3, 4, 5), np.int64)
    calls = [lambda lab, **kw: f3d.label_motion_sums(zero, zero, zero, lab, **kw),
             lambda lab, **kw: f3d.fit_label_motion(zero, zero, zero, lab, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="integers"):
            call(np.ones((3, 4, 5), F32))                     # labels are integers
        with pytest.raises(ValueError, match="int32"):
            call(good * 2 ** 31)
        with pytest.raises(ValueError, match="int32"):
            call(good * -(2 ** 31) - 1)
        with pytest.raises(ValueError, match="n_labels"):
            call(np.zeros((3, 4, 5), np.int32))               # labels.max() is 0: no body
        with pytest.raises(ValueError, match="n_labels"):
            call(good, n_labels=(1 << 22) + 1)
        with pytest.raises(ValueError, match="n_labels"):
            call(good * ((1 << 22) + 1))
        with pytest.raises(ValueError, match="integers"):
            call(np.ones((4, 5), np.int32))
    with pytest.raises(ValueError, match="model"):
        f3d.fit_label_motion(zero, zero, zero, good, model="similarity")
    bits, n = f3d._labels_as_float_bits(np.array([[[5, -1, 3]]], np.int16), None)
    assert n == 5 and bits.dtype == np.float32 and bits.view(np.int32).tolist() == [[[5, -1, 3]]]
    for name in ("label_motion_sums", "solve_label_motion", "fit_label_motion", "remove_label_motion", "LabelMotion"):
        assert callable(getattr(f3d, name))
    assert hasattr(f3d.OpticalFlow, "label_motion") and hasattr(f3d.OpticalFlow, "label_motion_end")
    motion = f3d.solve_label_motion((f3d.MotionSums * 3)(), (4, 4, 4))
    assert len(motion) == 3 and motion.rms_after is None and motion.centre.shape == (3, 3) and motion.matrix.shape == (3, 3, 3)
    assert [r["status"] for r in motion.as_table()] == ["empty"] * 3 and motion.as_table()[2]["label"] == 3


def test_a_library_without_one_entry_is_reported_by_that_entry(f3d, monkeypatch):
    """remove_label_motion resolves f3d_remove_label_motion before f3d_label_motion_sums, and the sums never ask for the other"""
    real = f3d._entry
    zero = np.zeros((3, 4, 5), F32)
    labels = np.ones((3, 4, 5), np.int32)
    motion = f3d.solve_label_motion((f3d.MotionSums * 1)(), (5, 4, 3))

    def without(missing):
        def entry(name, argtypes, what):
            if name == missing:
                raise f3d.F3dError(f"no {name}")
            return real(name, argtypes, what)
        return entry

    monkeypatch.setattr(f3d, "_entry", without("f3d_remove_label_motion"))
    with pytest.raises(f3d.F3dError, match="no f3d_remove_label_motion"):
        f3d.remove_label_motion(zero, zero, zero, labels, motion)
    with pytest.raises(ValueError, match="integers"):                     # the sums get past their entry to the argument checks
        f3d.label_motion_sums(zero, zero, zero, labels.astype(F32))
    monkeypatch.setattr(f3d, "_entry", without("f3d_label_motion_sums"))
    with pytest.raises(f3d.F3dError, match="no f3d_label_motion_sums"):
        f3d.label_motion_sums(zero, zero, zero, labels)


CASE = textwrap.dedent('''
    import ctypes as C, importlib, os, sys
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
    labels = np.ones((D, H, W), np.int32)
    motion = pkg.solve_label_motion((pkg.MotionSums * 1)(), (W, H, D))      # host code: runs here
    assert motion.status.tolist() == [1]
    sums, remove = "f3d_label_motion_sums", "f3d_remove_label_motion"
    for call, entry in ((lambda: flow.label_motion(labels), sums), (lambda: flow.label_motion(labels, model="affine"), sums),
                        (lambda: pkg.fit_label_motion(u, v, w, labels), sums), (lambda: pkg.label_motion_sums(u, v, w, labels), sums),
                        (lambda: pkg.remove_label_motion(u, v, w, labels, motion), remove)):
        try:
            call(); raise SystemExit("a call succeeded without " + entry)
        except pkg.F3dError as e:
            assert entry in str(e), str(e)
    flow.label_motion_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_label_motion_sums nor f3d_remove_label_motion: libf3d_host.so built against it must still
    load (RTLD_NOW) and solve flows, and the per-label calls must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_label_motion_sums" not in names and "f3d_remove_label_motion" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def _label_file(tmp_path, name, values):
    p = tmp_path / name
    np.asarray(values, np.int32).tofile(p)
    return str(p)


@pytest.mark.parametrize("case,needle", [("similarity", "usage"), ("no-model", "need each other"), ("no-labels", "need each other"),
                                         ("min-only", "need each other"), ("bad-min", "usage"), ("negative-min", "usage"),
                                         ("missing-value", "usage"), ("missing-file", "cannot read"), ("short-file", "cannot read"),
                                         ("no-body", "largest label"), ("too-many", "largest label"), ("partial", "--label-motion"),
                                         ("concurrent", "--label-motion"), ("sequence", "--cumulative")])
def test_flow3d_label_motion_argument_errors(tmp_path, case, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    good = _label_file(tmp_path, "labels.raw", np.ones(64))
    frames = paths if case == "sequence" else paths[:2]
    extra = {"similarity": ["--labels", good, "--label-motion", "similarity"],
             "no-model": ["--labels", good],
             "no-labels": ["--label-motion", "rigid"],
             "min-only": ["--label-min-voxels", "5"],
             "bad-min": ["--labels", good, "--label-motion", "rigid", "--label-min-voxels", "few"],
             "negative-min": ["--labels", good, "--label-motion", "rigid", "--label-min-voxels", "-3"],
             "missing-value": ["--labels", good, "--label-motion"],
             "missing-file": ["--labels", str(tmp_path / "nothing.raw"), "--label-motion", "rigid"],
             "short-file": ["--labels", _label_file(tmp_path, "short.raw", np.ones(63)), "--label-motion", "rigid"],
             "no-body": ["--labels", _label_file(tmp_path, "zero.raw", np.zeros(64)), "--label-motion", "rigid"],
             "too-many": ["--labels", _label_file(tmp_path, "many.raw", np.full(64, (1 << 22) + 1)), "--label-motion", "rigid"],
             "partial": ["--labels", good, "--label-motion", "rigid", "--partial"],
             "concurrent": ["--labels", good, "--label-motion", "affine", "--concurrent", "2"],
             "sequence": ["--labels", good, "--label-motion", "rigid"]}[case]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *frames, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--labels FILE --label-motion translation|rigid|affine [--label-min-voxels K]]" in run.stdout
    assert "[--detrend translation|rigid|affine [--detrend-min-zncc T]]" in run.stdout          # the earlier usage text is all still there
    assert "3D optical flow" not in run.stdout                                                   # before any device is touched
    assert not any("labelres" in n or "labelmotion" in n or "flow-" in n for n in os.listdir(tmp_path))
