"""The device reductions against exact references (tests/exact_ref.py): f3d_abs_max's contract (the largest FINITE |x| over the slab
window, NaN and +-Inf ignored), f3d_flow_stats and f3d_residual_stats (min / max exact, sums within 1e-12 of math.fsum) and the
statistics of f3d_flow_strain, on boxes inside larger containers and slab windows whose neighbouring planes, rows, columns and pitch
padding hold larger extremes, and at 512 x 512 x 64 with the extremes in the last wave, row group and run; the strain statistics'
determinism and their partial buffer growing and shrinking back."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from strain_ref import same_bits, strain_ref, strain_stats_ref
from subbox import SubBox, poison

pytestmark = pytest.mark.gpu

BIG = (512, 512, 64)


def abs_max(f3d, p, dims, slab=None):
    r = C.c_float()
    f3d.check(f3d.hip().f3d_abs_max(p, *dims, C.byref(slab) if slab is not None else None, C.byref(r)), "f3d_abs_max")
    return np.float32(r.value)


def flow_stats(f3d, ps, dims, slab=None):
    mn, mx, s = C.c_float(), C.c_float(), C.c_double()
    f3d.check(f3d.hip().f3d_flow_stats(*ps, *dims, C.byref(slab) if slab is not None else None, C.byref(mn), C.byref(mx),
                                       C.byref(s)), "f3d_flow_stats")
    return np.float32(mn.value), np.float32(mx.value), s.value


def residual_stats(f3d, p0, pw, dims, slab=None):
    ssq, sab, mx = C.c_double(), C.c_double(), C.c_float()
    f3d.check(f3d.hip().f3d_residual_stats(p0, pw, *dims, C.byref(slab) if slab is not None else None, C.byref(ssq), C.byref(sab),
                                           C.byref(mx)), "f3d_residual_stats")
    return ssq.value, sab.value, np.float32(mx.value)


def check_flow_stats(got, u, v, w):
    m = X.magnitude32(u, v, w)
    mn, mx, s = got
    assert mn == m.min() and mx == m.max(), (mn, m.min(), mx, m.max())
    exact = X.fsum(m.astype(np.float64))
    assert abs(s - exact) <= 1e-12 * exact, (s, exact)


def check_residual(got, f0, fw):
    d = (np.asarray(fw, np.float32) - np.asarray(f0, np.float32)).astype(np.float32)
    ssq, sab, mx = got
    assert mx == np.abs(d).max(), (mx, np.abs(d).max())
    d64 = d.astype(np.float64)
    e_sq, e_ab = X.fsum(d64 * d64), X.fsum(np.abs(d64))
    assert abs(ssq - e_sq) <= 1e-12 * e_sq and abs(sab - e_ab) <= 1e-12 * e_ab, (ssq, e_sq, sab, e_ab)


# ---- B: windows inside poisoned containers ------------------------------------------------------------------------------

# (level dims, slab (z_base, z_lo, z_hi) or None, container dims): the container holds planes z_base .. z_base + Dc - 1
WINDOWS = [((70, 9, 6), None, (131, 13, 9)), ((70, 9, 20), (5, 7, 15), (96, 12, 12)), ((256, 16, 8), (0, 3, 5), (300, 17, 8)),
           ((1, 1, 3), (1, 1, 2), (2, 2, 3)), ((513, 65, 4), (2, 3, 4), (520, 66, 3))]


def window_arrays(rng, sb, dims, slab, fill, lo, hi):
    """a full container array: `fill` everywhere, box values in [lo, hi) on the window's planes (container planes z - z_base) and
    every value outside the window made larger in magnitude than anything inside; returns (full, window view)"""
    w, h, d = dims
    z_base, z_lo, z_hi = slab if slab else (0, 0, d)
    full = poison(rng, sb.full, fill)
    a, b = z_lo - z_base, z_hi - z_base
    inside = rng.uniform(lo, hi, size=(b - a, h, w)).astype(np.float32)
    full[a:b, :h, :w] = inside
    if fill == "finite":
        # the neighbouring planes of the box (outside the window, inside the level) hold the largest values of all
        full[:a, :h, :w] = np.float32(5e4)
        full[b:, :h, :w] = np.float32(-6e4)
    return full, inside


@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("dims,slab,cdims", WINDOWS)
def test_reductions_see_only_the_window(f3d, dims, slab, cdims, fill):
    rng = np.random.default_rng(sum(dims) + (slab[1] if slab else 0))
    sl = f3d.Slab(*slab) if slab else None
    sb = SubBox(f3d, cdims)
    try:
        def put(lo, hi, plant=None):
            full, inside = window_arrays(rng, sb, dims, slab, fill, lo, hi)
            if plant is not None:
                plant(inside)
                z0 = (slab[1] - slab[0]) if slab else 0
                full[z0:z0 + inside.shape[0], :dims[1], :dims[0]] = inside
            p = sb.c.alloc()
            sb.c.upload(p, full)
            return p, inside

        def last_column_extreme(a):
            a[-1, -1, -1] = -2.75                # the extreme in the window's last voxel

        pf, f = put(-2, 2, last_column_extreme)
        assert abs_max(f3d, pf, dims, sl) == X.finite_abs_max(f)
        comps = [put(-4, 4) for _ in range(3)]
        check_flow_stats(flow_stats(f3d, [p for p, _ in comps], dims, sl), *[a for _, a in comps])
        (p0, f0), (pw, fw) = put(0, 255), put(0, 255)
        check_residual(residual_stats(f3d, p0, pw, dims, sl), f0, fw)
    finally:
        sb.free()


# ---- D: reductions at scale ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_box(f3d):
    """one 512 x 512 x 64 level in containers with two columns of pitch padding more and one more row and plane"""
    sb = SubBox(f3d, (BIG[0] + 2, BIG[1] + 1, BIG[2] + 1))
    yield sb
    sb.free()


@pytest.fixture
def big(big_box):
    big_box.set_current()
    return big_box


def release(sb, ps):
    for p in ps:
        sb.f3d.check(sb.f3d.hip().f3d_free(p), "f3d_free")
        sb.c._ptrs.remove(p)


def upload_big(sb, vol, rest=np.float32(0)):
    p = sb.c.alloc()
    full = np.full(sb.full, rest, np.float32)
    full[:BIG[2], :BIG[1], :BIG[0]] = vol
    sb.c.upload(p, full)
    return p


ABS_CASES = ["negative extreme and signed zeros", "denormals only", "all zeros", "nan and inf ignored", "larger outside",
             "extreme in the last wave"]


@pytest.mark.parametrize("case", ABS_CASES)
def test_abs_max_contract_at_scale(f3d, big, case):
    rng = np.random.default_rng(ABS_CASES.index(case))
    w, h, d = BIG
    vol = rng.uniform(-1, 1, size=(d, h, w)).astype(np.float32)
    rest = np.float32(0)
    sl = None
    if case == "negative extreme and signed zeros":
        vol[40, 300, 200] = -7.5
        vol[::7, ::5, ::3] = -0.0
        vol[1, 1, ::2] = 0.0
    elif case == "denormals only":
        vol = (rng.uniform(-1, 1, size=vol.shape) * 1e-39).astype(np.float32)
        vol[63, 511, 511] = np.float32(-1.1e-38)            # the largest subnormal magnitude planted in the very last voxel
        assert (np.abs(vol) < np.finfo(np.float32).tiny).all() and (vol != 0).any()
    elif case == "all zeros":
        vol[:] = 0
        vol[5, 5, 5] = -0.0
    elif case == "nan and inf ignored":
        vol[rng.random(vol.shape) < 0.01] = np.nan
        vol[0, 0, 0], vol[63, 511, 511], vol[32, 256, 448] = np.inf, -np.inf, np.nan
        vol[63, 511, 510] = -3.25
    elif case == "larger outside":
        rest = np.float32(9e3)                               # pitch padding, row H, plane D
        vol[0] = 50.0                                        # a plane outside the window
        vol[-1] = -60.0
        sl = big.f3d.Slab(0, 1, d - 1)
    else:
        vol[63, 511, 448 + 63] = 5.0                         # last lane of the last x-wave, last row group, last plane
        vol[63, 508, 448] = -5.5
    p = upload_big(big, vol, rest)
    try:
        window = vol if sl is None else vol[1:d - 1]
        got = abs_max(f3d, p, BIG, sl)
        want = X.finite_abs_max(window)
        assert got.view(np.uint32) == want.view(np.uint32), (case, got, want)
        if case == "denormals only":
            assert 0 < got < np.finfo(np.float32).tiny
    finally:
        release(big, [p])


def test_flow_and_residual_stats_at_scale(f3d, big):
    rng = np.random.default_rng(3)
    w, h, d = BIG
    comps = [rng.uniform(-4, 4, size=(d, h, w)).astype(np.float32) for _ in range(3)]
    # the largest and the smallest magnitude in the last x lane, the last row and the last plane
    for c in comps:
        c[63, 511, 511] = 9.0
        c[62, 510, 255] = 0.0
    comps[0][63, 300, 511] = 1e-20
    comps[1][63, 300, 511] = comps[2][63, 300, 511] = 0
    ps = [upload_big(big, c, np.float32(100)) for c in comps]
    f0 = rng.uniform(0, 255, size=(d, h, w)).astype(np.float32)
    fw = rng.uniform(0, 255, size=(d, h, w)).astype(np.float32)
    fw[63, 511, 511] = 1000.0
    p0, pw = upload_big(big, f0, np.float32(-1e4)), upload_big(big, fw, np.float32(1e4))
    try:
        check_flow_stats(flow_stats(f3d, ps, BIG), *comps)
        check_residual(residual_stats(f3d, p0, pw, BIG), f0, fw)
        sl = f3d.Slab(0, 5, 60)
        check_flow_stats(flow_stats(f3d, ps, BIG, sl), *[c[5:60] for c in comps])
        check_residual(residual_stats(f3d, p0, pw, BIG, sl), f0[5:60], fw[5:60])
    finally:
        release(big, ps + [p0, pw])


def strain_stats(f3d, sb, ins, dims):
    """the statistics of a call that stores eq alone (vol is computed for them all the same)"""
    eq = sb.sentinel()
    try:
        st = f3d.StrainStats()
        f3d.check(f3d._strain_entry()(*ins, (f3d._dp * 8)(0, 0, 0, 0, 0, 0, 0, eq), 4, *dims, C.byref(st)), "f3d_flow_strain")
    finally:
        release(sb, [eq])
    return st.as_dict()


def check_strain_stats(got, vol, eq):
    want = strain_stats_ref(vol, eq)
    for k in ("defined", "folded"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("vol_min", "vol_max", "eq_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])
    ok = ~np.isnan(vol)
    exact = X.fsum(vol[ok].astype(np.float64))
    assert abs(got["vol_sum"] - exact) <= 1e-12 * max(1.0, X.fsum(np.abs(vol[ok].astype(np.float64)))), (got["vol_sum"], exact)


def test_strain_statistics_at_scale(f3d, big):
    """extremes of vol and eq in the last x-wave, the last row group and the last z run; the result is the same bits twice"""
    rng = np.random.default_rng(4)
    w, h, d = BIG
    comps = X.smooth_displacement(BIG, "sine", amp=0.05, seed=9)
    # a bump of u at x = 500 in the last row group and run: G00 = +1.5 at x = 499 (the vol maximum), -1.5 at x = 501 (the minimum)
    comps[0][50, 510, 500] += np.float32(3.0)
    comps[1][rng.random(comps[1].shape) < 0.002] = np.nan
    want = strain_ref(*comps)
    vol = want["vol"]
    zmax, ymax, xmax = np.unravel_index(np.nanargmax(vol), vol.shape)
    zmin, ymin, xmin = np.unravel_index(np.nanargmin(vol), vol.shape)
    ze, ye, xe = np.unravel_index(np.nanargmax(want["eq"]), vol.shape)
    for z, y, x in ((zmax, ymax, xmax), (zmin, ymin, xmin), (ze, ye, xe)):
        assert x >= 448 and y >= 508 and z >= 32, (z, y, x)
    ins = [upload_big(big, c, np.float32(np.nan)) for c in comps]
    try:
        a = strain_stats(f3d, big, ins, BIG)
        b = strain_stats(f3d, big, ins, BIG)
        check_strain_stats(a, vol, want["eq"])
        assert np.float64(a["vol_sum"]).view(np.uint64) == np.float64(b["vol_sum"]).view(np.uint64)
        assert a == b or all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)
    finally:
        release(big, ins)


def one_defined(dims, at):
    """a NaN volume with exactly one defined voxel `at` = (x, y, z): it and its +x, +y, +z neighbours present"""
    w, h, d = dims
    comps = [np.full((d, h, w), np.nan, np.float32) for _ in range(3)]
    x, y, z = at
    for dz, dy, dx, val in ((0, 0, 0, 0.0), (0, 0, 1, 0.5), (0, 1, 0, -0.25), (1, 0, 0, 0.125)):
        for r, c in enumerate(comps):
            c[z + dz, y + dy, x + dx] = np.float32(val * (r + 1))
    return comps


def test_strain_statistics_of_one_defined_voxel_in_the_last_partial(f3d, big):
    w, h, d = BIG
    comps = one_defined(BIG, (w - 2, h - 2, d - 2))
    want = strain_ref(*comps)
    assert int((~np.isnan(want["vol"])).sum()) == 1
    ins = [upload_big(big, c, np.float32(np.nan)) for c in comps]
    try:
        st = strain_stats(f3d, big, ins, BIG)
        check_strain_stats(st, want["vol"], want["eq"])
        assert st["defined"] == 1 and st["vol_min"] == st["vol_max"] == st["vol_sum"]
    finally:
        release(big, ins)


def test_strain_partials_grow_and_shrink_back(f3d):
    """small, large, small: the thread's partial buffer is reallocated for the large volume and reused for the small one after it"""
    shapes = [(70, 9, 6), (700, 300, 70), (33, 5, 3)]
    for k, dims in enumerate(shapes):
        w, h, d = dims
        rng = np.random.default_rng(k)
        comps = X.smooth_displacement(dims, "quadratic", amp=0.05, seed=k)
        comps = X.with_holes(comps, *X.seam_holes(dims, rng, density=0.01))
        want = strain_ref(*comps)
        got = f3d.flow_strain(*comps, fields=("vol", "eq"))
        assert same_bits(got["vol"], want["vol"]) and same_bits(got["eq"], want["eq"]), dims
        check_strain_stats(got["stats"], want["vol"], want["eq"])
