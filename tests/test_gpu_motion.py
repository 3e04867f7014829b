"""The motion fit on the GPU: f3d_motion_sums and f3d_remove_motion against their numpy restatement (tests/motion_ref.py), never
against themselves, in NaN-poisoned containers larger than the box; the refusals of both entries; OpticalFlow.motion of a solved flow
against fit_motion + remove_motion by hand; and bin/flow3d --detrend in a pipelined sequence.

Bounds.  The coordinate sums are integers: equal to the restatement exactly.  A displacement sum of n binary64 terms differs from the
correctly rounded sum (math.fsum) by at most n 2^-53 sum |term| whatever the order of the additions, so nothing is measured.  On the
dyadic affine constructions every term and every partial sum is a multiple of 2^-10 below 2^43 (asserted here), hence exact in
binary64 in any order and in the factored form X * sum_z d as well: there the device must equal math.fsum bit for bit.  The residuals of
f3d_remove_motion have a fixed evaluation order: bit for bit.

Shapes: a wave covers 64 x, a workgroup 4 rows, a run 32 planes; the list has sizes of one, below, at and one above those, and
330 x 48 x 100, whose 6 * 12 * 4 = 288 workgroup partials make every thread of the fold merge at least one and some two."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as ref
from motion_ref import affine_field, holes, rotation

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
F32 = np.float32
U = 2.0 ** -53
SENTINEL = 0x7F      # byte fill of outputs: 0x7F7F7F7F = 3.39e38
WEIGHT_MIN = 0.75
SHAPES = [(1, 1, 1), (5, 1, 1), (64, 1, 1), (1, 1, 40), (7, 6, 5), (65, 5, 33), (70, 24, 20), (130, 9, 33), (330, 48, 100)]
CASES = ("noise", "holes", "weight", "absent")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def case_inputs(dims, case):
    """u, v, w (and a weight) of shape [d, h, w] for one of the four input kinds"""
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    u, v, ww = (rng.normal(m, 1.5, (d, h, w)).astype(F32) for m in (2.0, -1.0, 0.5))
    weight = None
    if case == "holes":
        pick = rng.random((d, h, w))
        u[pick < 0.04] = np.nan
        v[(pick >= 0.04) & (pick < 0.07)] = np.nan
        ww[(pick >= 0.07) & (pick < 0.10)] = np.nan
        for a in (u, v, ww):
            a[: max(1, d // 3), : max(1, h // 2), w - max(1, w // 4):] = np.nan          # a NaN block touching three faces
    elif case == "weight":
        weight = rng.choice(np.array([0.0, 0.5, WEIGHT_MIN, np.nextafter(F32(WEIGHT_MIN), F32(0)), 0.9, 1.0, np.nan, -np.inf, np.inf], F32),
                            size=(d, h, w))
        u[rng.random((d, h, w)) < 0.05] = np.nan
    elif case == "absent":
        weight = np.full((d, h, w), np.nan, F32)
        if w * h * d > 1:
            weight[0, 0, 0] = np.nextafter(F32(WEIGHT_MIN), F32(0))                         # just below: absent too
    return u, v, ww, weight


def device_sums(f3d, u, v, w, weight=None, weight_min=WEIGHT_MIN, calls=1):
    """f3d_motion_sums on a box in the corner of NaN-poisoned containers three columns, two rows and a plane larger"""
    d, h, w_ = u.shape
    fn, _ = f3d._motion_entry()
    box = f3d.Containers(w_ + 3, h + 2, d + 1)
    try:
        p = [box.new(a) for a in (u, v, w)]
        pw = box.new(weight) if weight is not None else 0
        box.set_current()
        out = []
        for _ in range(calls):
            s = f3d.MotionSums()
            f3d.check(fn(*p, pw, weight_min, w_, h, d, C.byref(s)), "f3d_motion_sums")
            out.append(s)
    finally:
        box.free()
    return out if calls > 1 else out[0]


def check_sums(got, want, exact_d=False):
    assert got.n == want["n"]
    assert list(got.Sx) == want["Sx"] and [2 * x for x in got.Sx] == want["x2"]               # exactly, as integers too
    assert list(got.Sxx) == want["Sxx"] and [4 * x for x in got.Sxx] == want["xx4"]
    for name, count in (("d", 3), ("xd", 9), ("dd", 3)):
        g, e, a = list(getattr(got, "S" + name)), want["S" + name], want["abs_" + name]
        for i in range(count):
            if exact_d:
                assert g[i] == e[i] and np.signbit(g[i]) == np.signbit(e[i]), (name, i, g[i], e[i])
            else:
                assert abs(g[i] - e[i]) <= want["n"] * U * a[i], (name, i, g[i], e[i], want["n"] * U * a[i])


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_sums_against_the_restatement(f3d, dims, case):
    w, h, d = dims
    u, v, ww, weight = case_inputs(dims, case)
    want = ref.motion_sums(u, v, ww, weight, WEIGHT_MIN)
    first, second = device_sums(f3d, u, v, ww, weight, calls=2)
    assert bytes(first) == bytes(second)                                     # two calls, identical bytes
    check_sums(first, want)
    n = w * h * d
    if case == "noise":                                                      # a full box: the closed forms
        assert first.n == n and list(first.Sx) == [0, 0, 0] and list(first.Sxx)[3:] == [0, 0, 0]
        assert [12 * x for x in list(first.Sxx)[:3]] == [n * (w * w - 1), n * (h * h - 1), n * (d * d - 1)]
    elif case == "absent":
        assert first.n == 0 and not any(first.Sx) and not any(first.Sxx) and not any(first.Sd) and not any(first.Sxd) and not any(first.Sdd)
    elif n > 100:
        assert 0 < first.n < n
    if case == "weight":                                                     # the value equal to weight_min is present, the one below is not
        at, below = weight == F32(WEIGHT_MIN), weight == np.nextafter(F32(WEIGHT_MIN), F32(0))
        m = ref.present_mask(u, v, ww, weight, WEIGHT_MIN)
        assert not m[below].any() and (n < 100 or (m[at].any() and below.any()))


def test_a_nan_weight_min_is_fine_without_a_weight_and_the_mask_is_binary(f3d):
    u, v, ww, _ = case_inputs((70, 24, 20), "noise")
    a = device_sums(f3d, u, v, ww, None, float("nan"))
    b = device_sums(f3d, u, v, ww, np.full(u.shape, 7.0, F32), 0.5)          # any weight at or above the minimum counts once
    assert bytes(a) == bytes(b) and a.n == u.size


@pytest.mark.parametrize("with_holes", [False, True], ids=["full", "holes"])
@pytest.mark.parametrize("dims", [(7, 6, 5), (70, 24, 20), (130, 9, 33)], ids=ids)
def test_sums_of_dyadic_fields_are_exact(f3d, dims, with_holes):
    w, h, d = dims
    rng = np.random.default_rng(w * 100 + h)
    M = rng.integers(-8, 9, (3, 3)) / 16.0
    t = rng.integers(-40, 41, 3) / 8.0
    exact = affine_field((d, h, w), M, t)
    field = [a.astype(F32) for a in exact]
    if with_holes:
        for a in field:
            a[holes((d, h, w), 5)] = np.nan
    # the construction: d is a multiple of 1/32, X of 1/2, so every term of every sum is a multiple of 2^-10, and the sums of the
    # absolute terms stay below 2^43: every partial sum in any order, and X * sum_z d, is a binary64 number
    m = ref.present_mask(*field)
    X = ref.centred_coordinates((d, h, w), m)
    for a, e in zip(field, exact):
        assert np.array_equal(a[m].astype(np.float64), e[m])
        assert np.array_equal(a[m].astype(np.float64) * 32, np.round(a[m].astype(np.float64) * 32))
    assert np.array_equal(X * 2, np.round(X * 2))
    want = ref.motion_sums(*field)
    assert max(want["abs_d"] + want["abs_xd"] + want["abs_dd"]) < 2.0 ** 43
    check_sums(device_sums(f3d, *field), want, exact_d=True)
    # and the fit of the device's sums is the construction
    fit = f3d.fit_motion(*field, model="affine")
    assert np.abs(fit.matrix - M).max() <= 1e-11 and np.abs(np.array(list(fit.t)) - t).max() <= 1e-11 and fit.n == int(m.sum())


def test_sums_refusals(f3d):
    hip = f3d.hip()
    fn, _ = f3d._motion_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w, m = (box.new(np.zeros((8, 8, 8), F32)) for _ in range(4))
        box.set_current()
        s = f3d.MotionSums()
        s.n = 77
        bad = [(0, v, w, 0, 0.5, 8, 8, 8, C.byref(s)), (u, 0, w, 0, 0.5, 8, 8, 8, C.byref(s)), (u, v, 0, m, 0.5, 8, 8, 8, C.byref(s)),
               (u, v, w, 0, 0.5, 8, 8, 8, None), (u, v, w, m, float("nan"), 8, 8, 8, C.byref(s)),
               (u, v, w, 0, 0.5, 0, 8, 8, C.byref(s)), (u, v, w, 0, 0.5, 8, 0, 8, C.byref(s)), (u, v, w, m, 0.5, 8, 8, 0, C.byref(s)),
               (u, v, w, 0, 0.5, 9, 8, 8, C.byref(s))]                       # larger than the container
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_motion_sums" in hip.f3d_last_error()
        assert s.n == 77                                                     # a refused call writes nothing
        assert fn(u, v, w, 0, float("nan"), 8, 8, 8, C.byref(s)) == 0 and s.n == 512
        assert fn(u, v, w, m, float("-inf"), 8, 8, 8, C.byref(s)) == 0 and s.n == 512
    finally:
        box.free()


# ---- the subtraction ---------------------------------------------------------------------------------------------------------------------------

def make_fit(f3d, dims, kind):
    w, h, d = dims
    fit = f3d.MotionFit()
    fit.centre[:] = [(w - 1) / 2, (h - 1) / 2, (d - 1) / 2]
    rng = np.random.default_rng(5)
    if kind == "large":
        fit.t[:] = [3.2, -1.5, 0.7]
        fit.M[:] = list(rng.uniform(-0.3, 0.3, 9))
    elif kind == "tiny":
        fit.t[:] = [1e-7, -3e-8, 2e-9]
        fit.M[:] = list(rng.uniform(-1e-9, 1e-9, 9))
    else:                                                                    # a rotation about a centre that is no half-integer
        fit.centre[:] = [1.3, 0.1, -2.7]
        fit.t[:] = [0.0, 12.5, -0.001]
        fit.M[:] = list((rotation(0.4, (3, -1, 2)) - np.eye(3)).ravel())
    return fit


def device_remove(f3d, u, v, w, fit, in_place, stats=True):
    """f3d_remove_motion in larger containers: the three whole output containers and the statistics"""
    d, h, w_ = u.shape
    cdims = (w_ + 3, h + 2, d + 1)
    _, fn = f3d._motion_entry()
    box = f3d.Containers(*cdims)
    try:
        p = [box.new(a) for a in (u, v, w)]
        outs = p if in_place else [box.alloc(fill=SENTINEL) for _ in range(3)]
        box.set_current()
        st = f3d.MotionResidual() if stats else None
        f3d.check(fn(*p, *outs, C.byref(fit), w_, h, d, st), "f3d_remove_motion")
        f3d.sync()
        full = [box.download(o, cdims) for o in outs]
        ins = [box.download(a, cdims) for a in p]
    finally:
        box.free()
    return full, ins, (st.as_dict() if stats else None)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_residual_stats(st, st_want):
    """the statistics of a residual: the count and the float32 maximum exactly, the binary64 sum of squares within
    3 n 2^-53 of its own size (a square and two additions per voxel, in any order)"""
    assert st["present"] == st_want["present"]
    if st_want["present"]:
        assert F32(st["max_abs"]) == F32(st_want["max_abs"])
    else:
        assert np.isnan(st["max_abs"])
    assert abs(st["sum_sq"] - st_want["sum_sq"]) <= 3 * st_want["present"] * U * st_want["sum_sq"]


@pytest.mark.parametrize("kind", ["large", "tiny", "rotation"])
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_remove_equals_the_restatement_bit_for_bit(f3d, dims, kind):
    w, h, d = dims
    u, v, ww, _ = case_inputs(dims, "holes")
    fit = make_fit(f3d, dims, kind)
    want = ref.remove_motion(u, v, ww, list(fit.centre), list(fit.t), list(fit.M))
    st_want = want[3]
    inside = np.zeros((d + 1, h + 2, w + 3), bool)
    inside[:d, :h, :w] = True
    for in_place in (False, True):
        full, ins, st = device_remove(f3d, u, v, ww, fit, in_place)
        for got, exp, src, name in zip(full, want, (u, v, ww), "uvw"):
            assert np.array_equal(bits(got[:d, :h, :w]), bits(exp)), f"{dims} {kind} in_place={in_place} {name}: " \
                f"{int((bits(got[:d, :h, :w]) != bits(exp)).sum())} of {exp.size} differ"
            assert np.array_equal(np.isnan(got[:d, :h, :w]), np.isnan(src))                          # NaN in, NaN out, and only there
            pad = 0xFFFFFFFF if in_place else 0x7F7F7F7F
            assert (bits(got)[~inside] == pad).all(), "written outside the box"
        if not in_place:
            for kept, src in zip(ins, (u, v, ww)):
                assert np.array_equal(bits(kept[:d, :h, :w]), bits(src))                              # the inputs are not touched
        check_residual_stats(st, st_want)
    full, _, st = device_remove(f3d, u, v, ww, fit, False, stats=False)                              # without statistics: the same field
    assert all(np.array_equal(bits(g[:d, :h, :w]), bits(e)) for g, e in zip(full, want)) and st is None


def test_remove_statistics_of_a_volume_with_nothing_present(f3d):
    nan = np.full((3, 4, 5), np.nan, F32)
    zero = np.zeros((3, 4, 5), F32)
    ru, rv, rw, st = f3d.remove_motion(zero, nan, zero, make_fit(f3d, (5, 4, 3), "large"))
    assert st["present"] == 0 and st["sum_sq"] == 0 and np.isnan(st["max_abs"])
    assert np.isnan(rv).all() and not np.isnan(ru).any() and not np.isnan(rw).any()                 # per component


def test_remove_refusals(f3d):
    hip = f3d.hip()
    _, fn = f3d._motion_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w = (box.new(np.ones((8, 8, 8), F32)) for _ in range(3))
        o = [box.alloc(fill=SENTINEL) for _ in range(3)]
        box.set_current()
        good = make_fit(f3d, (8, 8, 8), "large")

        def broken(field, index, value):
            f = make_fit(f3d, (8, 8, 8), "large")
            getattr(f, field)[index] = value
            return f

        bad = [(0, v, w, *o, good), (u, v, w, o[0], 0, o[2], good), (u, v, w, *o, None),
               (u, v, w, v, o[1], o[2], good), (u, v, w, o[0], u, o[2], good), (u, v, w, v, u, o[2], good),   # an output on another input
               (u, v, w, o[0], o[0], o[2], good), (u, v, w, o[0], o[1], o[0], good),                            # two outputs alike
               (u, u, w, *o, good),                                                                            # two inputs alike
               (u, v, w, *o, broken("M", 4, float("nan"))), (u, v, w, *o, broken("t", 2, float("inf"))),
               (u, v, w, *o, broken("centre", 0, float("-inf")))]
        for args in bad:
            fit = args[6]
            assert fn(*args[:6], C.byref(fit) if fit is not None else None, 8, 8, 8, None) != 0, args
            assert b"f3d_remove_motion" in hip.f3d_last_error()
        assert fn(u, v, w, *o, C.byref(good), 0, 8, 8, None) != 0 and b"f3d_remove_motion" in hip.f3d_last_error()
        f3d.sync()
        for p in o:
            assert (bits(box.download(p, (8, 8, 8))) == 0x7F7F7F7F).all()                                   # nothing was written
        for p in (u, v, w):
            assert (box.download(p, (8, 8, 8)) == 1).all()
        assert fn(u, v, w, u, v, w, C.byref(good), 8, 8, 8, None) == 0                                      # in place
        assert fn(u, v, w, u, o[1], w, C.byref(good), 8, 8, 8, None) == 0                                   # and partly in place
        f3d.sync()
    finally:
        box.free()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def fit_fields(fit):
    d = fit.as_dict()
    return [d[k] for k in ("centre", "t", "matrix", "n", "rms_before", "cos_angle", "axial", "model")]


def test_motion_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        with pytest.raises(f3d.F3dError, match="match"):                        # a mask needs the zncc of a match of this pair
            flow.motion(model="rigid", min_zncc=0.8)
        for model in ("rigid", "affine", "translation"):
            got = flow.motion(model=model)
            hand = f3d.fit_motion(u, v, ww, model=model)
            assert fit_fields(got["fit"]) == fit_fields(hand), model           # bit for bit: == of every number
            ru, rv, rw, st = f3d.remove_motion(u, v, ww, hand)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((got["u"], got["v"], got["w"]), (ru, rv, rw)))
            assert got["stats"] == st and st["present"] == w * h * d
            rms_after = np.sqrt(st["sum_sq"] / st["present"])
            print(f"{model}: t {list(hand.t)}, rms {hand.rms_before:.4f} -> {rms_after:.4f}")
            assert rms_after <= hand.rms_before
            # and both are what the restatement gives: its sums through the same solve, its subtraction of that fit
            s = ref.motion_sums(u, v, ww)
            sums = f3d.MotionSums()
            sums.n = s["n"]
            for name in ("Sx", "Sxx", "Sd", "Sxd", "Sdd"):
                getattr(sums, name)[:] = s[name]
            want = f3d.solve_motion(sums, (w, h, d), model)
            assert np.allclose(list(hand.t), list(want.t), rtol=0, atol=1e-9) and np.allclose(hand.matrix, want.matrix, rtol=0, atol=1e-10)
            exp = ref.remove_motion(u, v, ww, list(hand.centre), list(hand.t), list(hand.M))
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((ru, rv, rw), exp[:3]))
        assert list(hand.centre) == [(w - 1) / 2, (h - 1) / 2, (d - 1) / 2]
        # the translation model is the mean of the flow
        tr = f3d.fit_motion(u, v, ww, model="translation")
        assert np.allclose(list(tr.t), [a.astype(np.float64).mean() for a in (u, v, ww)], rtol=0, atol=1e-12) and not tr.matrix.any()
        m = flow.match(fields="zncc")
        masked = flow.motion(model="rigid", min_zncc=0.8)
        with np.errstate(invalid="ignore"):
            count = int((m["zncc"] >= F32(0.8)).sum())
        assert masked["fit"].n == count and 0 < count < w * h * d
        by_hand = f3d.fit_motion(u, v, ww, model="rigid", weight=m["zncc"], weight_min=0.8)
        assert fit_fields(masked["fit"]) == fit_fields(by_hand)
        assert masked["stats"]["present"] == w * h * d                          # the mask selects what is fitted, not what is subtracted
        # a new solve makes the old zncc stale
        flow.compute_resident(silent=True, **KW)
        with pytest.raises(f3d.F3dError, match="match"):
            flow.motion(model="rigid", min_zncc=0.8)
        # the trajectory is a source too, but has no mask
        flow.trajectory_begin()
        flow.trajectory_append()
        traj = flow.motion(source="trajectory", model="rigid")
        assert fit_fields(traj["fit"]) == fit_fields(f3d.fit_motion(u, v, ww, model="rigid"))
        flow.match(fields="zncc")
        with pytest.raises(f3d.F3dError, match="trajectory"):
            flow.motion(source="trajectory", min_zncc=0.8)
        flow.motion_end()
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), (u, v, ww)))
    finally:
        flow.destroy()


# ---- bin/flow3d --detrend in a pipelined sequence --------------------------------------------------------------------------------------------

LINE = re.compile(r"motion frame (\d+) -> frame (\d+) \(rigid\): t \((\S+), (\S+), (\S+)\), angle (\S+) deg about \((\S+), (\S+), (\S+)\), "
                  r"rms (\S+) -> (\S+), max \|res\| (\S+), (\d+) of (\d+) voxels")


def test_cli_detrend_in_a_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    frames = [s0, s1, s0]
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    total = w * h * d
    read = lambda name: np.fromfile(str(tmp_path / name), F32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    so = run("d", ["--detrend", "rigid", "--cumulative", "--strain", "vol"])
    plain = run("p", ["--cumulative", "--strain", "vol"])
    lines = LINE.findall(so)
    assert len(lines) == 2
    for k in range(2):
        for name in [f"flow-{c}" for c in "uvw"] + [f"disp-{c}" for c in "uvw"] + ["strain-vol"]:
            assert raw(f"d_{k}_{name}{suffix}") == raw(f"p_{k}_{name}{suffix}"), f"{name} of pair {k}"
        disp = [read(f"d_{k}_disp-{c}{suffix}") for c in "uvw"]
        fit = f3d.fit_motion(*disp, model="rigid")
        res = f3d.remove_motion(*disp, fit)
        for c, exp in zip("uvw", res[:3]):
            assert np.array_equal(bits(read(f"d_{k}_detrended-{c}{suffix}")), bits(exp)), f"detrended-{c} of pair {k}"
        m = lines[k]
        assert (int(m[0]), int(m[1])) == (0, k + 1) and int(m[12]) == fit.n and int(m[13]) == total
        for txt, val in zip(m[2:5], fit.t):
            assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12)
        sine = float(np.linalg.norm(list(fit.axial)))
        assert float(m[5]) == pytest.approx(np.degrees(np.arctan2(sine, fit.cos_angle)), rel=1e-4, abs=1e-9)
        assert float(m[9]) == pytest.approx(fit.rms_before, rel=1e-5)
        assert float(m[10]) == pytest.approx(np.sqrt(res[3]["sum_sq"] / res[3]["present"]), rel=1e-5)
        assert float(m[11]) == pytest.approx(res[3]["max_abs"], rel=1e-5)
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("strain frame", "displacement frame"))]
    assert keep(so) == keep(plain) and len(keep(so)) == 4
    assert not any(n.startswith("p_") and "detrended" in n for n in os.listdir(tmp_path))

    # the pair's own flow, fitted where the pair's zncc is at least 0.8; affine prints the matrix
    so = run("z", ["--match", "zncc", "--detrend", "rigid", "--detrend-min-zncc", "0.8"])
    lines = LINE.findall(so)
    assert len(lines) == 2
    for k in range(2):
        zncc = read(f"z_{k}_match-zncc{suffix}")
        flow_k = [read(f"z_{k}_flow-{c}{suffix}") for c in "uvw"]
        with np.errstate(invalid="ignore"):
            assert int(lines[k][12]) == int((zncc >= F32(0.8)).sum())
        fit = f3d.fit_motion(*flow_k, model="rigid", weight=zncc, weight_min=0.8)
        for c, exp in zip("uvw", f3d.remove_motion(*flow_k, fit)[:3]):
            assert np.array_equal(bits(read(f"z_{k}_detrended-{c}{suffix}")), bits(exp)), f"masked detrended-{c} of pair {k}"
        assert (int(lines[k][0]), int(lines[k][1])) == (k, k + 1)
    so = run("a", ["--detrend", "affine"])
    assert len(re.findall(r"motion frame \d+ -> frame \d+ \(affine\): t \(.*\), M \((?:\S+, \S+, \S+;? ?){3}\), rms", so)) == 2
