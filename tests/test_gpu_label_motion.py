"""The per-label motion on the GPU: f3d_label_motion_sums and f3d_remove_label_motion against their numpy restatement
(tests/label_motion_ref.py), never against themselves, in poisoned containers larger than the box; the refusals of both entries;
fit_label_motion of a field with one rigid motion per cell against the solve of the restatement's sums; OpticalFlow.label_motion; and
bin/flow3d --labels --label-motion in a pipelined sequence.

Bounds.  The sums are exact integers rounded once: every field of every label equals the restatement bit for bit, whatever the
schedule, and two calls give the same bytes.  The residuals have a fixed evaluation order: bit for bit.  One label everywhere is also
compared with f3d_motion_sums, whose d-sums are of the unquantised float32 displacement: |q 2^-14 - d| <= 2^-15 per voxel, so
|Sd - Sd'| <= n 2^-15, |Sxd_ij - Sxd_ij'| <= 2^-15 sum |X_i| and |Sdd_j - Sdd_j'| <= sum (2^-14 |d_j| + 2^-30), each plus
tests/test_gpu_motion.py's bound n 2^-53 sum |term| of a binary64 sum in any order.

Shapes: a wave covers 64 x, a workgroup 4 rows, a run 32 planes; 65 x 5 x 33 is one past a tile along every axis and 130 x 9 x 70 has three
tiles in x and z.  The LDS table has 128 slots, so the 1000 random labels of "random" overflow it in every full tile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import label_motion_ref as ref
import motion_ref
from motion_ref import rotation
from test_gpu_motion import check_residual_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
U = 2.0 ** -53
SENTINEL = 0x7F      # byte fill of outputs: 0x7F7F7F7F = 3.39e38
WEIGHT_MIN = 0.75
SHAPES = [(1, 1, 1), (3, 2, 2), (65, 5, 33), (130, 9, 70)]
LAYOUTS = ("one", "voronoi", "random", "spare", "outside")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def label_volume(dims, layout):
    """(labels [d, h, w] int32, n_labels) of one of the five layouts"""
    w, h, d = dims
    rng = np.random.default_rng(w * 31 + h)
    if layout == "one":
        return np.ones((d, h, w), np.int32), 1
    if layout == "random":                                   # more labels than the LDS table has slots
        return rng.integers(1, 1001, (d, h, w)).astype(np.int32), 1000
    lab = ref.voronoi((d, h, w), 40, seed=w)
    if layout == "voronoi":
        return lab, 40
    if layout == "spare":                                    # n_labels larger than any label used
        return lab, 57
    pick = rng.random((d, h, w))                             # background, negative and too large
    lab[pick < 0.10] = 0
    lab[(pick >= 0.10) & (pick < 0.14)] = -3
    lab[(pick >= 0.14) & (pick < 0.18)] = 41
    lab[(pick >= 0.18) & (pick < 0.20)] = np.iinfo(np.int32).max
    lab[(pick >= 0.20) & (pick < 0.22)] = np.iinfo(np.int32).min
    lab[(pick >= 0.22) & (pick < 0.24)] = 0x7FC00000         # the bits of a float NaN are a label like any other
    return lab, 40


def values(dims, with_weight):
    """u, v, w (and a weight): full-scale noise, NaN holes and a NaN block, ties of both signs, denormals, the edge of the range"""
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d + with_weight)
    u, v, ww = (rng.uniform(-1023.0, 1023.0, (d, h, w)).astype(F32) for _ in range(3))
    k = rng.integers(-2 ** 23, 2 ** 23, (d, h, w))
    ties = ((k + 0.5) / 16384.0).astype(F32)                 # exact in float32: 2k + 1 is below 2^24
    assert np.array_equal(ties.astype(np.float64) * 16384.0, k + 0.5)
    pick = rng.random((d, h, w))
    u[pick < 0.10] = ties[pick < 0.10]
    v[(pick >= 0.10) & (pick < 0.20)] = ties[(pick >= 0.10) & (pick < 0.20)]
    specials = np.array([1e-40, -1e-40, 1.4e-45, 0.0, -0.0, 1023.99994, -1023.99994, 1024.0, -1024.0, np.inf, -np.inf,
                         0.5 / 16384, -0.5 / 16384, 1.5 / 16384, -1.5 / 16384, 2.5 / 16384], F32)
    assert specials[5] == np.nextafter(F32(1024), F32(0))
    for a, lo in ((u, 0.20), (v, 0.26), (ww, 0.32)):
        m = (pick >= lo) & (pick < lo + 0.06)
        a[m] = rng.choice(specials, size=int(m.sum()))
    u[(pick >= 0.40) & (pick < 0.43)] = np.nan
    v[(pick >= 0.43) & (pick < 0.45)] = np.nan
    ww[(pick >= 0.45) & (pick < 0.47)] = np.nan
    if w * h * d > 100:
        for a in (u, v, ww):
            a[: max(1, d // 3), : max(1, h // 2), w - max(1, w // 4):] = np.nan          # a NaN block touching three faces
    weight = None
    if with_weight:
        weight = rng.choice(np.array([0.0, 0.5, WEIGHT_MIN, np.nextafter(F32(WEIGHT_MIN), F32(0)), 0.9, 1.0, np.nan, -np.inf, np.inf], F32),
                            size=(d, h, w))
    return u, v, ww, weight


def device_sums(f3d, u, v, w, labels, n_labels, weight=None, weight_min=WEIGHT_MIN, calls=1):
    """f3d_label_motion_sums on a box in the corner of containers three columns, two rows and a plane larger, the floats poisoned
    with NaN and the labels with -1 (foreign): (sums array, info dict) per call"""
    d, h, w_ = u.shape
    fn, _ = f3d._label_motion_entry()
    box = f3d.Containers(w_ + 3, h + 2, d + 1)
    try:
        p = [box.new(a) for a in (u, v, w)]
        pl = box.new(np.ascontiguousarray(labels, np.int32).view(F32))
        pw = box.new(weight) if weight is not None else 0
        box.set_current()
        out = []
        for _ in range(calls):
            s = (f3d.MotionSums * n_labels)()
            info = f3d.LabelInfo()
            f3d.check(fn(*p, pl, n_labels, pw, weight_min, w_, h, d, s, C.byref(info)), "f3d_label_motion_sums")
            out.append((s, info.as_dict()))
    finally:
        box.free()
    return out if calls > 1 else out[0]


def fbits(x):
    return np.array(x, np.float64).view(np.uint64).tolist()


def check_sums(got, want):
    assert len(got) == len(want)
    for L, (g, e) in enumerate(zip(got, want), 1):
        assert g.n == e["n"], (L, g.n, e["n"])
        for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
            assert fbits(list(getattr(g, name))) == fbits(e[name]), (L, name, list(getattr(g, name)), e[name])   # the sign of zero too


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_weight", [False, True], ids=["plain", "weight"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_sums_equal_the_restatement_bit_for_bit(f3d, dims, layout, with_weight):
    w, h, d = dims
    labels, n_labels = label_volume(dims, layout)
    u, v, ww, weight = values(dims, with_weight)
    want, info_want = ref.label_sums(u, v, ww, labels, n_labels, weight, WEIGHT_MIN)
    (first, info), (second, info2) = device_sums(f3d, u, v, ww, labels, n_labels, weight, calls=2)
    assert bytes(first) == bytes(second) and info == info2               # two calls, identical bytes
    assert info == info_want
    check_sums(first, want)
    assert sum(s.n for s in first) == info["used"]
    if w * h * d > 100:
        assert info["absent"] and info["out_of_range"] and info["used"]
        assert (info["background"] > 0 and info["foreign"] > 0) == (layout == "outside")
        if layout == "spare":
            assert all(s.n == 0 and bytes(s) == bytes(f3d.MotionSums()) for s in list(first)[40:])   # a label with no voxel: all +0


def test_both_limbs_and_the_arithmetic_shift(f3d):
    """130 x 9 x 70 of one label with |d| = 1023.99 of mixed sign: Idd exceeds 2^63, Id and Ixd are of both signs"""
    w, h, d = 130, 9, 70
    rng = np.random.default_rng(3)
    u, v, ww = (np.where(rng.random((d, h, w)) < p, F32(1023.99), F32(-1023.99)).astype(F32) for p in (0.5, 0.2, 0.9))
    labels = np.ones((d, h, w), np.int32)
    ints, _ = ref.label_integers(u, v, ww, labels, 1)
    assert min(ints[0]["Idd"]) > 2 ** 63 and min(ints[0]["Id"]) < 0 < max(ints[0]["Id"])
    assert min(ints[0]["Ixd"]) < -2 ** 32 and max(ints[0]["Ixd"]) > 2 ** 32
    want, info_want = ref.label_sums(u, v, ww, labels, 1)
    got, info = device_sums(f3d, u, v, ww, labels, 1)
    check_sums(got, want)
    assert info == info_want and info["used"] == w * h * d


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_one_label_everywhere_is_f3d_motion_sums_of_the_quantised_field(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w)
    u, v, ww = (rng.normal(m, 1.5, (d, h, w)).astype(F32) for m in (2.0, -1.0, 0.5))
    u[rng.random((d, h, w)) < 0.05] = np.nan
    weight = rng.choice(np.array([0.5, WEIGHT_MIN, 1.0, np.nan], F32), size=(d, h, w))
    got, info = device_sums(f3d, u, v, ww, np.ones((d, h, w), np.int32), 1, weight)
    got = got[0]
    sums_fn, _ = f3d._motion_entry()
    box = f3d.Containers(w + 3, h + 2, d + 1)
    try:
        p = [box.new(a) for a in (u, v, ww, weight)]
        box.set_current()
        whole = f3d.MotionSums()
        f3d.check(sums_fn(*p, WEIGHT_MIN, w, h, d, C.byref(whole)), "f3d_motion_sums")
    finally:
        box.free()
    assert got.n == whole.n == info["used"] and list(got.Sx) == list(whole.Sx) and list(got.Sxx) == list(whole.Sxx)
    r = motion_ref.motion_sums(u, v, ww, weight, WEIGHT_MIN)
    m = motion_ref.present_mask(u, v, ww, weight, WEIGHT_MIN)
    X = np.abs(motion_ref.centred_coordinates((d, h, w), m)).sum(axis=0)
    n = r["n"]
    # The issue's bound for the d-sums, n 2^-15 plus the any-order bound, is what Sd is held to.  It cannot hold for the other two: a
    # term of Sxd is X_i d_j and moves by up to |X_i| 2^-15 under the quantisation, a term of Sdd is d_j^2 and moves by up to
    # 2 |d_j| 2^-15 + 2^-30.  Their bounds are those figures summed over the voxels, from the quantisation step alone, plus the same
    # any-order bound.
    for j in range(3):
        assert abs(got.Sd[j] - whole.Sd[j]) <= n * 2.0 ** -15 + n * U * r["abs_d"][j]
        assert abs(got.Sdd[j] - whole.Sdd[j]) <= 2.0 ** -14 * r["abs_d"][j] + n * 2.0 ** -30 + n * U * r["abs_dd"][j]
        for i in range(3):
            assert abs(got.Sxd[3 * i + j] - whole.Sxd[3 * i + j]) <= 2.0 ** -15 * X[i] + n * U * r["abs_xd"][3 * i + j]


def test_sums_refusals(f3d):
    hip = f3d.hip()
    fn, _ = f3d._label_motion_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w, m = (box.new(np.zeros((8, 8, 8), F32)) for _ in range(4))
        lab = box.new(np.ones((8, 8, 8), np.int32).view(F32))
        box.set_current()
        s = (f3d.MotionSums * 2)()
        s[0].n = 77
        info = f3d.LabelInfo()
        info.used = 55
        tail = (8, 8, 8, s, C.byref(info))
        bad = [(0, v, w, lab, 2, 0, 0.5, *tail), (u, 0, w, lab, 2, 0, 0.5, *tail), (u, v, 0, lab, 2, m, 0.5, *tail),
               (u, v, w, 0, 2, 0, 0.5, *tail), (u, v, w, lab, 2, 0, 0.5, 8, 8, 8, None, C.byref(info)),
               (u, v, w, lab, 0, 0, 0.5, *tail), (u, v, w, lab, (1 << 22) + 1, 0, 0.5, *tail),
               (u, v, w, lab, 2, m, float("nan"), *tail),
               (u, v, w, lab, 2, 0, 0.5, 0, 8, 8, s, None), (u, v, w, lab, 2, 0, 0.5, 8, 0, 8, s, None), (u, v, w, lab, 2, m, 0.5, 8, 8, 0, s, None),
               (u, v, w, lab, 2, 0, 0.5, 9, 8, 8, s, None),                  # larger than the container
               # too large for the 64-bit coordinate sums, refused by the entry itself whatever the container holds: above 32768 along
               # an axis, and above 2^33 voxels with every axis within 32768
               (u, v, w, lab, 2, 0, 0.5, 32769, 1, 1, s, None), (u, v, w, lab, 2, 0, 0.5, 1, 32769, 1, s, None),
               (u, v, w, lab, 2, 0, 0.5, 1, 1, 32769, s, None), (u, v, w, lab, 2, 0, 0.5, 32768, 32768, 9, s, None)]
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_label_motion_sums" in hip.f3d_last_error()
            if args[7] * args[8] * args[9] > 2 ** 20:
                assert b"exceeds 32768 along an axis or 2^33 voxels" in hip.f3d_last_error()
        assert s[0].n == 77 and info.used == 55                              # a refused call writes nothing
        assert fn(u, v, w, lab, 2, 0, float("nan"), 8, 8, 8, s, None) == 0 and s[0].n == 512 and s[1].n == 0   # info is optional
        assert fn(u, v, w, lab, 2, m, float("-inf"), *tail) == 0 and s[0].n == 512 and info.used == 512
    finally:
        box.free()


# ---- the subtraction ---------------------------------------------------------------------------------------------------------------------------

def make_fits(f3d, dims, n_labels):
    """fits and status of n_labels labels: large, tiny and rotation fits in turn, every fifth label not OK"""
    w, h, d = dims
    fits, status = (f3d.MotionFit * n_labels)(), (C.c_int * n_labels)()
    rng = np.random.default_rng(5)
    for i in range(n_labels):
        fit = fits[i]
        fit.centre[:] = list(rng.uniform(0, 1, 3) * np.array([w, h, d]))
        if i % 3 == 0:
            fit.t[:] = [3.2, -1.5, 0.7]
            fit.M[:] = list(rng.uniform(-0.3, 0.3, 9))
        elif i % 3 == 1:
            fit.t[:] = [1e-7, -3e-8, 2e-9]
            fit.M[:] = list(rng.uniform(-1e-9, 1e-9, 9))
        else:                                                                # a rotation about a centre outside the volume
            fit.centre[:] = [1.3, 0.1, -2.7]
            fit.t[:] = [0.0, 12.5, -0.001]
            fit.M[:] = list((rotation(0.4, (3, -1, 2)) - np.eye(3)).ravel())
        status[i] = (0, 1, 2, 3)[(i // 5) % 4] if i % 5 == 4 else 0
        if status[i] != 0 and i % 2:
            fit.t[0] = float("nan")                                           # what a fit that is not OK holds is not looked at
    return fits, status


def fit_arrays(fits, status):
    return ([list(f.centre) for f in fits], [list(f.t) for f in fits], [list(f.M) for f in fits], [s == 0 for s in status])


def device_remove(f3d, u, v, w, labels, fits, status, in_place, stats=True):
    """f3d_remove_label_motion in larger containers: the three whole output containers, the inputs afterwards and the statistics"""
    d, h, w_ = u.shape
    cdims = (w_ + 3, h + 2, d + 1)
    _, fn = f3d._label_motion_entry()
    box = f3d.Containers(*cdims)
    try:
        p = [box.new(a) for a in (u, v, w)]
        pl = box.new(np.ascontiguousarray(labels, np.int32).view(F32))
        outs = p if in_place else [box.alloc(fill=SENTINEL) for _ in range(3)]
        box.set_current()
        st = f3d.MotionResidual() if stats else None
        f3d.check(fn(*p, pl, len(fits), fits, status, *outs, w_, h, d, st), "f3d_remove_label_motion")
        f3d.sync()
        full = [box.download(o, cdims) for o in outs]
        ins = [box.download(a, cdims) for a in p + [pl]]
    finally:
        box.free()
    return full, ins, (st.as_dict() if stats else None)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("layout", ["one", "outside", "random"])
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_remove_equals_the_restatement_bit_for_bit(f3d, dims, layout):
    w, h, d = dims
    labels, n_labels = label_volume(dims, layout)
    rng = np.random.default_rng(w + 1)
    u, v, ww = (rng.normal(m, 1.5, (d, h, w)).astype(F32) for m in (2.0, -1.0, 0.5))
    pick = rng.random((d, h, w))
    u[pick < 0.04] = np.nan
    v[(pick >= 0.04) & (pick < 0.07)] = np.nan
    fits, status = make_fits(f3d, dims, n_labels)
    want = ref.remove_label_motion(u, v, ww, labels, *fit_arrays(fits, status))
    st_want = want[3]
    ok = np.array([s == 0 for s in status])
    valid = (labels >= 1) & (labels <= n_labels)
    valid &= ok[np.where(valid, labels - 1, 0)]
    inside = np.zeros((d + 1, h + 2, w + 3), bool)
    inside[:d, :h, :w] = True
    for in_place in (False, True):
        full, ins, st = device_remove(f3d, u, v, ww, labels, fits, status, in_place)
        for got, exp, src, name in zip(full, want, (u, v, ww), "uvw"):
            assert np.array_equal(bits(got[:d, :h, :w]), bits(exp)), f"{dims} {layout} in_place={in_place} {name}: " \
                f"{int((bits(got[:d, :h, :w]) != bits(exp)).sum())} of {exp.size} differ"
            assert np.array_equal(np.isnan(got[:d, :h, :w]), np.isnan(src) | ~valid)       # NaN in, NaN out; NaN where there is no fit
            pad = 0xFFFFFFFF if in_place else 0x7F7F7F7F
            assert (bits(got)[~inside] == pad).all(), "written outside the box"
        if not in_place:
            for kept, src in zip(ins[:3], (u, v, ww)):
                assert np.array_equal(bits(kept[:d, :h, :w]), bits(src))                    # the inputs are not touched
        assert np.array_equal(bits(ins[3][:d, :h, :w]), labels.view(np.uint32)) and (bits(ins[3])[~inside] == 0xFFFFFFFF).all()
        check_residual_stats(st, st_want)
    full, _, st = device_remove(f3d, u, v, ww, labels, fits, status, False, stats=False)   # without statistics: the same field
    assert all(np.array_equal(bits(g[:d, :h, :w]), bits(e)) for g, e in zip(full, want)) and st is None


def test_remove_refusals(f3d):
    hip = f3d.hip()
    _, fn = f3d._label_motion_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w = (box.new(np.ones((8, 8, 8), F32)) for _ in range(3))
        lab = box.new(np.ones((8, 8, 8), np.int32).view(F32))
        o = [box.alloc(fill=SENTINEL) for _ in range(3)]
        box.set_current()
        good, status = make_fits(f3d, (8, 8, 8), 2)

        def broken(field, index, value):
            f, _ = make_fits(f3d, (8, 8, 8), 2)
            getattr(f[1], field)[index] = value
            return f

        dims = (8, 8, 8, None)
        bad = [(0, v, w, lab, 2, good, status, *o, *dims), (u, v, w, 0, 2, good, status, *o, *dims),
               (u, v, w, lab, 2, good, status, o[0], 0, o[2], *dims), (u, v, w, lab, 2, None, status, *o, *dims),
               (u, v, w, lab, 2, good, None, *o, *dims), (u, v, w, lab, 0, good, status, *o, *dims),
               (u, v, w, lab, (1 << 22) + 1, good, status, *o, *dims),
               (u, v, w, lab, 2, good, status, v, o[1], o[2], *dims), (u, v, w, lab, 2, good, status, o[0], u, o[2], *dims),   # an output on another input
               (u, v, w, lab, 2, good, status, o[0], o[0], o[2], *dims), (u, v, w, lab, 2, good, status, o[0], o[1], o[0], *dims),  # two outputs alike
               (u, u, w, lab, 2, good, status, *o, *dims),                                                              # two inputs alike
               (u, v, w, lab, 2, good, status, o[0], lab, o[2], *dims), (u, v, lab, lab, 2, good, status, *o, *dims),   # the labels among them
               (u, v, w, lab, 2, broken("M", 4, float("nan")), status, *o, *dims),
               (u, v, w, lab, 2, broken("t", 2, float("inf")), status, *o, *dims),
               (u, v, w, lab, 2, broken("centre", 0, float("-inf")), status, *o, *dims),
               (u, v, w, lab, 2, good, status, *o, 0, 8, 8, None), (u, v, w, lab, 2, good, status, *o, 9, 8, 8, None)]
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_remove_label_motion" in hip.f3d_last_error()
        f3d.sync()
        for p in o:
            assert (bits(box.download(p, (8, 8, 8))) == 0x7F7F7F7F).all()                                   # nothing was written
        for p in (u, v, w):
            assert (box.download(p, (8, 8, 8)) == 1).all()
        not_ok = (C.c_int * 2)(0, 3)                                         # a non-finite entry of a fit that is not OK is not looked at
        assert fn(u, v, w, lab, 2, broken("M", 4, float("nan")), not_ok, *o, *dims) == 0
        assert fn(u, v, w, lab, 2, good, status, u, v, w, *dims) == 0        # in place
        assert fn(u, v, w, lab, 2, good, status, u, o[1], w, *dims) == 0     # and partly in place
        f3d.sync()
    finally:
        box.free()


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------------

def cell_field(dims, seeds=12, noise=0.02):
    """labels of `seeds` Voronoi cells and a displacement that is a different rigid motion in every cell plus noise"""
    w, h, d = dims
    labels = ref.voronoi((d, h, w), seeds, seed=2)
    rng = np.random.default_rng(11)
    field = [np.zeros((d, h, w)) for _ in range(3)]
    truth = []
    for L in range(1, seeds + 1):
        R = rotation(rng.uniform(-0.08, 0.08), rng.normal(size=3))
        t = rng.uniform(-4, 4, 3)
        truth.append((R, t))
        whole = motion_ref.affine_field((d, h, w), R - np.eye(3), t)
        for a, b in zip(field, whole):
            a[labels == L] = b[labels == L]
    field = [(a + rng.normal(0, noise, a.shape)).astype(F32) for a in field]
    return labels, field, truth


def test_fit_label_motion_is_the_solve_of_the_restatements_sums(f3d):
    dims = (70, 24, 40)
    w, h, d = dims
    labels, field, truth = cell_field(dims)
    labels[:2, :3, :4] = 0                                   # some background
    labels[labels == 5] = 0                                  # an empty label
    labels[0, 0, 10:20] = 13                                 # a small one: ten voxels of a line
    got = f3d.fit_label_motion(*field, labels.astype(np.int64), model="rigid", n_labels=14, min_voxels=27)
    want_sums, info = ref.label_sums(*field, labels, 14)
    sums = (f3d.MotionSums * 14)()
    for s, e in zip(sums, want_sums):
        s.n = e["n"]
        for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
            getattr(s, name)[:] = e[name]
    want = f3d.solve_label_motion(sums, dims, "rigid", 27)
    assert got.info == info and info["background"] == int((labels == 0).sum())
    for name in ("status", "n", "centre", "t", "matrix", "cos_angle", "axial", "rms_before"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name          # the same sums feed the same host code
    assert got.status.tolist() == [0] * 4 + [ref.EMPTY] + [0] * 7 + [ref.SMALL, ref.EMPTY]
    for L, (R, t) in enumerate(truth, 1):
        if got.status[L - 1] == 0:
            assert np.abs(got.matrix[L - 1] + np.eye(3) - R).max() < 2e-3, L
    # the subtraction leaves the noise, per label, and NaN where there is no fit
    ru, rv, rw, st = f3d.remove_label_motion(*field, labels, got)
    exp = ref.remove_label_motion(*field, labels, got.centre, got.t, got.matrix, got.status == 0)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((ru, rv, rw), exp[:3]))
    fitted = np.isin(labels, 1 + np.flatnonzero(got.status == 0))
    assert np.array_equal(np.isnan(ru), ~fitted) and st["present"] == int(fitted.sum())
    ok = got.status == 0
    assert np.isnan(got.rms_after[~ok]).all()
    assert (got.rms_after[ok] < 0.06).all() and (got.rms_after[ok] > 0.02).all() and (got.rms_before[ok] > 0.1).all()
    after, _ = ref.label_sums(ru, rv, rw, labels, 14)
    for i in np.flatnonzero(ok):
        assert got.rms_after[i] == np.sqrt(((after[i]["Sdd"][0] + after[i]["Sdd"][1]) + after[i]["Sdd"][2]) / after[i]["n"])
    table = got.as_table()
    assert len(table) == 14 and table[4]["status"] == "empty" and table[0]["label"] == 1 and table[0]["rms_after"] == got.rms_after[0]


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
MOTION_FIELDS = ("status", "n", "centre", "t", "matrix", "cos_angle", "axial", "rms_before", "rms_after")


def same_motion(a, b):
    return all(np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True) for name in MOTION_FIELDS)


def test_label_motion_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    labels = ref.voronoi((d, h, w), 9, seed=6)
    labels[:, :2, :] = 0
    labels[3, 5, 7:11] = 10                                  # four voxels: small
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        with pytest.raises(f3d.F3dError, match="labels"):                       # nothing uploaded yet
            flow.label_motion(None, n_labels=10)
        for model in ("rigid", "affine", "translation"):
            got = flow.label_motion(labels if model == "rigid" else None, model=model, n_labels=11)   # uploaded once and kept
            hand = f3d.fit_label_motion(u, v, ww, labels, model=model, n_labels=11)
            ru, rv, rw, st = f3d.remove_label_motion(u, v, ww, labels, hand)
            assert same_motion(got["motion"], hand), model
            assert got["motion"].info == hand.info and hand.info["background"] == int((labels == 0).sum())
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((got["u"], got["v"], got["w"]), (ru, rv, rw)))
            assert hand.status.tolist() == [0] * 9 + [ref.SMALL, ref.EMPTY]
            assert (hand.rms_after[:9] <= hand.rms_before[:9]).all() and np.isnan(hand.rms_after[9:]).all()
            print(f"{model}: rms {hand.rms_before[:9].round(4).tolist()} -> {hand.rms_after[:9].round(4).tolist()}")
        with pytest.raises(ValueError):
            flow.label_motion(labels[:, :, :-1])
        # the trajectory is a source too
        flow.trajectory_begin()
        flow.trajectory_append()
        traj = flow.label_motion(labels, source="trajectory", model="rigid", n_labels=11)
        hand = f3d.fit_label_motion(u, v, ww, labels, n_labels=11)
        f3d.remove_label_motion(u, v, ww, labels, hand)
        assert same_motion(traj["motion"], hand)
        flow.label_motion_end()
        with pytest.raises(f3d.F3dError, match="labels"):                       # the labels went with the containers
            flow.label_motion(None, n_labels=11)
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), (u, v, ww)))
    finally:
        flow.destroy()


# ---- bin/flow3d --labels --label-motion in a pipelined sequence ------------------------------------------------------------------------------

LINE = re.compile(r"label motion frame (\d+) -> frame (\d+) \(rigid\): (\d+) labels fitted, (\d+) empty, (\d+) small, (\d+) degenerate; "
                  r"median \|t\| (\S+), max angle (\S+) deg, (\d+) foreign, (\d+) out of range voxels")


def test_cli_label_motion_in_a_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([s0, s1, s0]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    labels = ref.voronoi((d, h, w), 7, seed=1)
    labels[:2] = 0
    labels[5, 5, 5] = -4                                     # foreign
    labels[6, 6, 6:9] = 9                                    # label 8 is empty, label 9 small
    label_path = str(tmp_path / "labels.raw")
    labels.astype("<i4").tofile(label_path)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), F32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    so = run("l", ["--cumulative", "--strain", "vol", "--labels", label_path, "--label-motion", "rigid"])
    plain = run("p", ["--cumulative", "--strain", "vol"])
    lines = LINE.findall(so)
    assert len(lines) == 2 and not LINE.findall(plain)
    for k in range(2):
        for name in [f"flow-{c}" for c in "uvw"] + [f"disp-{c}" for c in "uvw"] + ["strain-vol"]:
            assert raw(f"l_{k}_{name}{suffix}") == raw(f"p_{k}_{name}{suffix}"), f"{name} of pair {k}"
        disp = [read(f"l_{k}_disp-{c}{suffix}") for c in "uvw"]
        motion = f3d.fit_label_motion(*disp, labels, model="rigid", n_labels=9)
        res = f3d.remove_label_motion(*disp, labels, motion)
        for c, exp in zip("uvw", res[:3]):
            assert np.array_equal(bits(read(f"l_{k}_labelres-{c}{suffix}")), bits(exp)), f"labelres-{c} of pair {k}"
        m = lines[k]
        status = motion.status.tolist()
        assert (int(m[0]), int(m[1])) == (0, k + 1)
        assert [int(x) for x in m[2:6]] == [status.count(s) for s in (0, 1, 2, 3)] == [7, 1, 1, 0]
        ok = motion.status == 0
        assert float(m[6]) == pytest.approx(np.median(np.linalg.norm(motion.t[ok], axis=1)), rel=1e-5)
        angle = np.degrees(np.arctan2(np.linalg.norm(motion.axial[ok], axis=1), motion.cos_angle[ok]))
        assert float(m[7]) == pytest.approx(angle.max(), rel=1e-4, abs=1e-9)
        assert int(m[8]) == motion.info["foreign"] == 1 and int(m[9]) == motion.info["out_of_range"]
        rows = open(tmp_path / f"l_{k}_labelmotion.csv").read().strip().split("\n")
        assert rows[0] == "label,status,n,cx,cy,cz,tx,ty,tz,angle_deg,ax,ay,az,rms_before,rms_after" and len(rows) == 10
        for i, row in enumerate(rows[1:]):
            cells = row.split(",")
            assert int(cells[0]) == i + 1 and cells[1] == f3d.LABEL_STATUS[status[i]] and int(cells[2]) == motion.n[i]
            got = np.array([float(c) for c in cells[3:9]])
            assert np.allclose(got, np.concatenate([motion.centre[i], motion.t[i]]), rtol=1e-8, atol=1e-12)
            assert float(cells[13]) == pytest.approx(motion.rms_before[i], rel=1e-8)
            if status[i] == 0:
                assert float(cells[9]) == pytest.approx(angle[list(np.flatnonzero(ok)).index(i)], rel=1e-6, abs=1e-9)
                assert float(cells[14]) == pytest.approx(motion.rms_after[i], rel=1e-8)
            else:
                assert np.isnan(float(cells[14]))
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("strain frame", "displacement frame"))]
    assert keep(so) == keep(plain) and len(keep(so)) == 4
    assert not any(n.startswith("p_") and "label" in n for n in os.listdir(tmp_path))
    # a single pair needs no --cumulative: the pair's grid is frame 0's; affine writes the matrix, three voxels in a row are degenerate
    r = subprocess.run(args[:-1] + ["--out", str(tmp_path / "a"), "--labels", label_path, "--label-motion", "affine",
                                    "--label-min-voxels", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"label motion frame 0 -> frame 1 \(affine\): 7 labels fitted, 1 empty, 0 small, 1 degenerate; median \|t\| \S+, 1 foreign",
                     r.stdout), r.stdout[-800:]
    rows = open(tmp_path / "a_labelmotion.csv").read().strip().split("\n")
    assert rows[0].startswith("label,status,n,cx,cy,cz,tx,ty,tz,m00,m01,m02,m10,") and len(rows) == 10 and len(rows[1].split(",")) == 20


