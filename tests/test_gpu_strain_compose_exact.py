"""f3d_flow_strain and f3d_compose_flow against independent references (tests/exact_ref.py) as well as their float32 restatements:
boxes inside larger containers whose outside (pitch padding included) holds finite values that would change the answer and then NaN,
the seams of the strain kernel's tiling (x = 63 / 64, y = 3 / 4, z = 31 / 32) and thin shapes, and one container over 4 GiB."""
import numpy as np
import pytest

import exact_ref as X
from strain_ref import NAMES, same_bits, strain_ref, strain_stats_ref
from subbox import SENTINEL_BITS, SubBox, outside, poison
from trajectory_ref import compose_ref

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 2, 2, 2, 2, 2, 4)


def run_strain(f3d, sb, ins, outs, mask, dims, stats):
    st = f3d.StrainStats() if stats else None
    arr = [p if mask & g else 0 for p, g in zip(outs, GROUPS)]
    f3d.check(f3d._strain_entry()(*ins, (f3d._dp * 8)(*arr), mask, *dims, st), "f3d_flow_strain")
    f3d.sync()
    return None if st is None else st.as_dict()


def check_stats_exact(got, vol, eq):
    """counts and extremes exact, the double sum within 1e-12 of the exact sum of the defined vol values"""
    want = strain_stats_ref(vol, eq)
    for k in ("defined", "folded"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("vol_min", "vol_max", "eq_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])
    ok = ~np.isnan(vol)
    exact = X.fsum(vol[ok].astype(np.float64))
    assert abs(got["vol_sum"] - exact) <= 1e-12 * max(1.0, X.fsum(np.abs(vol[ok].astype(np.float64)))), (got["vol_sum"], exact)


def check_header(got, comps, names=NAMES):
    """got (dict of float32 arrays) against the float64 header strain of comps: undefined set, values within the rounding bound"""
    G, und = X.gradient64(*comps)
    want = X.strain64(G, und)
    tol = X.strain_tolerance(G)
    ok = ~und
    for n in names:
        assert np.array_equal(np.isnan(got[n]), und), f"{n}: undefined set"
        if n == "eq":
            assert np.all(np.abs(got[n][ok].astype(np.float64) ** 2 - want[n][ok] ** 2) <= tol["eq2"][ok]), n
        else:
            assert np.all(np.abs(got[n][ok] - want[n][ok]) <= tol["vol" if n == "vol" else "e"][ok]), n


def check_affine(got, A, dims, und, names=NAMES):
    """defined voxels of an affine displacement hold the closed form exactly (vol, E) and within EQ_ULPS (eq)"""
    A0 = [[0.0 if dims[c] == 1 else A[r][c] for c in range(3)] for r in range(3)]
    cf = X.closed_form_fraction(A0)
    for n in names:
        assert np.array_equal(np.isnan(got[n]), und), f"{n}: undefined set"
        if n == "eq":
            assert (X.ulps_apart(got[n][~und], X.eq_of_E({k: float(cf[k]) for k in NAMES[1:7]})) <= X.EQ_ULPS).all()
        else:
            assert (got[n][~und] == np.float32(float(cf[n]))).all(), n


# ---- B: sub-boxes in poisoned containers ----------------------------------------------------------------------------------

SUB_CASES = [((37, 21, 9), (64, 32, 16)), ((64, 4, 32), (65, 5, 33)), ((65, 5, 33), (130, 8, 34)), ((1, 1, 1), (3, 2, 2)),
             ((63, 3, 2), (64, 4, 3))]


@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("kind", ["affine", "smooth"])
@pytest.mark.parametrize("dims,cdims", SUB_CASES)
def test_strain_of_a_box_inside_a_larger_container(f3d, dims, cdims, kind, fill):
    w, h, d = dims
    rng = np.random.default_rng(w * 131 + h * 7 + d)
    if kind == "affine":
        A, b = X.STRAIN_AFFINE[1]
        comps = X.affine_field(A, b, dims)
    else:
        comps = X.smooth_displacement(dims, "sine", amp=0.2, seed=w + h + d)
    all_nan, one_nan = X.seam_holes(dims, rng, density=0.03)
    comps = X.with_holes(comps, all_nan, one_nan, which=0)
    und = X.predicted_undefined(all_nan | one_nan)
    want = strain_ref(*comps)
    sb = SubBox(f3d, cdims)
    try:
        ins = [sb.put(c, poison(rng, sb.full, fill)) for c in comps]
        outs = [sb.sentinel() for _ in range(8)]
        mask_out = outside(np.empty(sb.full), dims)
        for mask, stats in ((7, True), (1, False), (2, True), (4, False), (5, True), (6, False)):
            for p in outs:
                f3d.check(f3d.hip().f3d_memset2d(p, sb.c.pitch, 0x7F, sb.c.pitch, cdims[1] * cdims[2]))
            st = run_strain(f3d, sb, ins, outs, mask, dims, stats)
            got = {}
            for i, (p, g) in enumerate(zip(outs, GROUPS)):
                full = sb.get(p)
                if mask & g:
                    assert (full.view(np.uint32)[mask_out] == SENTINEL_BITS).all(), (mask, NAMES[i], "written outside the box")
                    got[NAMES[i]] = full[:d, :h, :w]
                    assert same_bits(got[NAMES[i]], want[NAMES[i]]), (mask, NAMES[i], fill)
                else:
                    assert (full.view(np.uint32) == SENTINEL_BITS).all(), (mask, NAMES[i], "unselected output written")
            if kind == "affine":
                check_affine(got, A, dims, und, names=list(got))
            else:
                check_header(got, comps, names=list(got))
            if st is not None:
                check_stats_exact(st, want["vol"], want["eq"])
    finally:
        sb.free()


def random_step(rng, dims):
    """acc with points that stay, points exactly on 0 and n - 1, points that leave through every face, NaN; inc of a few voxels"""
    w, h, d = dims
    shape = (d, h, w)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    acc = [rng.uniform(-1.5, 1.5, size=shape).astype(np.float32) for _ in range(3)]
    pick = rng.random(shape)
    for a, c, n in zip(acc, (x, y, z), (w, h, d)):
        a[(pick > 0.5) & (pick < 0.6)] = (-c[(pick > 0.5) & (pick < 0.6)]).astype(np.float32)
        a[(pick > 0.6) & (pick < 0.7)] = (n - 1 - c[(pick > 0.6) & (pick < 0.7)]).astype(np.float32)
        a[pick > 0.95] += np.float32(n)
    acc[2][(pick > 0.9) & (pick < 0.91)] = np.nan
    inc = [rng.uniform(-2, 2, size=shape).astype(np.float32) for _ in range(3)]
    inc[1][rng.random(shape) < 0.005] = np.nan
    return acc, inc


def compose_box(f3d, sb, acc, inc, dims, fill, rng):
    """one f3d_compose_flow step of a box in sb's containers; returns (new acc box, lost, whole acc containers)"""
    pa = [sb.put(a, poison(rng, sb.full, fill)) for a in acc]
    before = [sb.get(p) for p in pa]
    pi = [sb.put(a, poison(rng, sb.full, fill)) for a in inc]
    import ctypes as C
    lost = C.c_ulonglong()
    f3d.check(f3d._compose_entry()(*pa, *pi, *dims, C.byref(lost)), "f3d_compose_flow")
    after = [sb.get(p) for p in pa]
    w, h, d = dims
    m = outside(before[0], dims)
    for b4, af in zip(before, after):
        assert np.array_equal(b4.view(np.uint32)[m], af.view(np.uint32)[m]), "written outside the box"
    return [a[:d, :h, :w] for a in after], int(lost.value)


@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("dims,cdims", SUB_CASES)
def test_compose_of_a_box_inside_a_larger_container(f3d, dims, cdims, fill):
    w, h, d = dims
    rng = np.random.default_rng(w * 17 + h * 5 + d)
    sb = SubBox(f3d, cdims)
    try:
        # exact: the affine steps one after the other, each from the exact result of the step before
        want = X.compose_affine_expected(X.COMPOSE_AFFINE, dims)
        acc = [np.zeros((d, h, w), np.float32)] * 3
        for k, (A, b) in enumerate(X.COMPOSE_AFFINE):
            inc = X.affine_field(A, b, dims)
            got, lost = compose_box(f3d, sb, acc, inc, dims, fill, rng)
            ref = compose_ref(acc, inc)
            for c in range(3):
                assert same_bits(got[c], ref[c]), (k, c, "restatement")
                assert same_bits(got[c], want[k][c]), (k, c, "exact")
            assert lost == int(np.isnan(want[k][0]).sum())
            acc = list(want[k])
        # random: faces, NaN, NaN samples
        acc, inc = random_step(rng, dims)
        got, lost = compose_box(f3d, sb, acc, inc, dims, fill, rng)
        ref = compose_ref(acc, inc)
        for c in range(3):
            assert same_bits(got[c], ref[c]), (c, "random step")
        assert lost == int(np.isnan(ref[0]).sum())
    finally:
        sb.free()


# ---- C: seam shapes ---------------------------------------------------------------------------------------------------------

SEAMS = [(1, 1, 2), (1, 5, 33), (63, 1, 1), (63, 4, 31), (64, 3, 32), (64, 4, 33), (64, 5, 65), (65, 1, 32), (65, 4, 2),
         (65, 5, 31), (127, 3, 33), (127, 5, 1), (129, 4, 65), (129, 1, 31), (129, 5, 32), (1, 4, 65), (127, 4, 2), (63, 5, 65),
         (64, 1, 1), (129, 3, 2)]


@pytest.mark.parametrize("dims", SEAMS)
def test_strain_on_the_seams_of_the_tiling(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w * 1009 + h * 101 + d)
    comps = X.smooth_displacement(dims, "quadratic", amp=0.05, seed=w + 3 * h + 7 * d)
    comps = X.with_holes(comps, *X.seam_holes(dims, rng, density=0.02), which=1)
    # single NaN voxels right on the seams (x 62..65, y 3 / 4, z 30..33) and on every face corner
    for x in (0, 62, 63, 64, 65, w - 1):
        for y in (0, 3, 4, h - 1):
            for z in (0, 30, 31, 32, 33, d - 1):
                if x < w and y < h and z < d and rng.random() < 0.3:
                    comps[int(rng.integers(0, 3))][z, y, x] = np.nan
    want = strain_ref(*comps)
    cdims = (w + 3, h + 2, d + 1)
    sb = SubBox(f3d, cdims)
    try:
        ins = [sb.put(c, poison(rng, sb.full, "finite")) for c in comps]
        outs = [sb.sentinel() for _ in range(8)]
        st = run_strain(f3d, sb, ins, outs, 7, dims, True)
        got = {}
        for n, p in zip(NAMES, outs):
            full = sb.get(p)
            assert (full.view(np.uint32)[outside(full, dims)] == SENTINEL_BITS).all(), n
            got[n] = full[:d, :h, :w]
            assert same_bits(got[n], want[n]), n
        check_header(got, comps)
        check_stats_exact(st, want["vol"], want["eq"])
        assert st["defined"] == int((~X.predicted_undefined(X.missing_mask(*comps))).sum())
    finally:
        sb.free()


@pytest.mark.parametrize("dims", SEAMS)
def test_compose_on_the_seams_of_the_tiling(f3d, dims):
    w, h, d = dims
    rng = np.random.default_rng(w * 2003 + h * 13 + d)
    sb = SubBox(f3d, (w + 2, h + 1, d + 1))
    try:
        want = X.compose_affine_expected(X.COMPOSE_AFFINE[:2], dims)
        acc = [np.zeros((d, h, w), np.float32)] * 3
        for k, (A, b) in enumerate(X.COMPOSE_AFFINE[:2]):
            got, lost = compose_box(f3d, sb, acc, X.affine_field(A, b, dims), dims, "finite", rng)
            for c in range(3):
                assert same_bits(got[c], want[k][c]), (k, c)
            assert lost == int(np.isnan(want[k][0]).sum())
            acc = list(want[k])
        acc, inc = random_step(rng, dims)
        got, lost = compose_box(f3d, sb, acc, inc, dims, "nan", rng)
        ref = compose_ref(acc, inc)
        for c in range(3):
            assert same_bits(got[c], ref[c]), c
        assert lost == int(np.isnan(ref[0]).sum())
    finally:
        sb.free()


# ---- E: one container over 4 GiB ---------------------------------------------------------------------------------------

def test_strain_and_compose_in_a_container_over_4_gib(f3d):
    """1024 x 1024 x 1025 (4.3 GB per container): strain of an exact affine displacement (vol only, with statistics) and one
    composition step of exact affine flows, generated, uploaded and checked against the closed forms by chunks of planes"""
    import ctypes as C
    dims = W, H, D = 1024, 1024, 1025
    N = W * H * D
    A1, b1 = X.COMPOSE_AFFINE[0]
    A2, b2 = X.COMPOSE_AFFINE[1]
    assert X.prove_compose_exact(X.COMPOSE_AFFINE[:2], dims)
    box = f3d.Containers(W, H, D)
    try:
        acc = [box.alloc() for _ in range(3)]
        inc = [box.alloc() for _ in range(3)]
        vol = box.alloc(fill=0x7F)
        assert box.pitch * H * D > 4 << 30
        box.set_current()
        step = 64
        for z0 in range(0, D, step):
            z1 = min(D, z0 + step)
            for p, a in zip(acc, X.affine_field(A1, b1, dims, z0, z1)):
                box.upload(p, a, plane0=z0)
            for p, a in zip(inc, X.affine_field(A2, b2, dims, z0, z1)):
                box.upload(p, a, plane0=z0)
        # strain of the step-1 displacement: G = A1 everywhere (faces are exact one-sided differences), no holes
        st = f3d.StrainStats()
        f3d.check(f3d._strain_entry()(*acc, (f3d._dp * 8)(vol, 0, 0, 0, 0, 0, 0, 0), 1, W, H, D, C.byref(st)), "f3d_flow_strain")
        cf = X.closed_form_fraction(A1)
        v = np.float32(float(cf["vol"]))
        assert float(v) == cf["vol"]
        assert st.defined == N and st.folded == 0 and st.vol_min == v and st.vol_max == v
        eq_bits = strain_ref(*X.affine_field(A1, b1, (3, 3, 3)))["eq"][1, 1, 1]
        assert np.float32(st.eq_max) == eq_bits
        assert st.vol_sum == float(cf["vol"]) * N          # every addend equal and dyadic: the double sum is exact
        for z0 in range(0, D, 128):
            z1 = min(D, z0 + 128)
            got = box.download(vol, (W, H, z1 - z0), plane0=z0)
            assert (got == v).all(), f"vol planes {z0}..{z1}"
        # one composition step from the step-1 displacement
        lost = C.c_ulonglong()
        f3d.check(f3d._compose_entry()(*acc, *inc, W, H, D, C.byref(lost)), "f3d_compose_flow")
        n_lost = 0
        for z0 in range(0, D, step):
            z1 = min(D, z0 + step)
            want = X.compose_affine_expected(X.COMPOSE_AFFINE[:2], dims, z0, z1)[1]
            for c in range(3):
                got = box.download(acc[c], (W, H, z1 - z0), plane0=z0)
                assert same_bits(got, want[c]), f"compose planes {z0}..{z1} component {c}"
            n_lost += int(np.isnan(want[0]).sum())
        assert lost.value == n_lost and 0 < n_lost < N
    finally:
        box.free()
