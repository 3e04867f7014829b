"""The three streaming operations of the pyramid loop stated from their definitions in binary64, the float32 rounding bounds that
separate a correct float32 kernel from them, and the inputs the tests of those operations share.

TEST INFRASTRUCTURE ONLY.  The oracle (oracle/f3d_oracle.c) restates the reference's kernels operation by operation, and the GPU
tests ask the device for the oracle's bits; whatever the oracle gets wrong they inherit.  The functions here are written from what
the operation MEANS, not from the oracle (tests/exact_ref.py does the same for the reductions), on dense numpy volumes [z, y, x]:

  resample_axis   output i of m along an axis of n cells is the mean of the piecewise-constant input over [i n / m, (i + 1) n / m).
                  The quotient is exact: in units of 1 / m cell j covers [j m, (j + 1) m) and window i covers [i n, (i + 1) n), their
                  overlap is an integer, and the weight of cell j is overlap / n.
  conv_axis       zero-padded, out[i] = sum_{j = -R .. R} k[R - j] s[i + j]  (include/f3d.h, f3d_conv_*; k as uploaded, in binary64).
  warp            trilinear backward warp.  The float32 coordinates x + u * (1 / hx) and the inside test are those of include/f3d.h and
                  k_warp (they decide WHICH cells are read, so they are part of the definition and are formed here with numpy's
                  float32 operations, one rounding each like the kernel's); the interpolation is binary64.  frame_0 where the point is
                  outside [0, n - 1] along any axis or not a number.

Rounding bounds (first order, u = 2^-24 the unit roundoff of binary32, |.| the largest magnitude of the input volume):

  resampling   |device - exact| <= 8 u (m + cnt) max|s|,  cnt = ceil(n / m) + 1 the most cells a window touches.
      The kernel integrates s over [left_f, right_f] with left_f = fl(i fl(n / m)): two roundings of a number <= n, so each window end is
      off by <= 2 u n, and forming an end fraction (l + 1) - left_f rounds once more, <= u.  The integral of a piecewise-constant s is
      Lipschitz in its ends with constant max|s| (a window end that crosses a cell boundary under this error trades a sliver of one
      cell for a sliver of the next), so both ends cost <= (4 n + 2) u max|s|.  The cnt products and cnt additions of
      value = value + s frac cost <= (cnt + 1) u sum|s frac| <= (cnt + 1) u (n / m) max|s|.  fl(m / n) and the last product cost 2 u of
      the result, <= 2 u max|s|.  After the normalisation m / n:  (4 m + 2 m / n + cnt + 3) u max|s| <= 8 (m + cnt) u max|s| for every
      n, m, cnt >= 1.  (A kernel that takes a wrong cell or a wrong fraction is off by order max|s|.)
  convolution  |device - exact| <= 1 u (2 R + 2) sum|k| max|s|.
      2 R + 1 products, one rounding each, added in sequence (the first addition, to 0, is exact): every product passes through at
      most 2 R + 1 roundings, error <= gamma_{2R+1} sum|k s|, and (2 R + 2) u exceeds gamma_{2R+1} = (2 R + 1) u / (1 - (2 R + 1) u)
      for R <= 25.
  warp         |device - exact| <= 10 u max|f1|.
      The coordinates are the same float32 numbers on both sides and the fractions d = x_f - floor(x_f) are exact.  1 - d rounds once;
      a corner weight (1 - dx)(1 - dy) and its product with f1 round twice more: <= 4 u per term of a plane's bilinear sum, whose
      weights add up to 1; its three additions cost <= 3 u max|f1|.  (1 - dz) v0 + dz v1 adds the rounding of 1 - dz, one product and
      one addition: (4 + 3) + 2 + 1 = 10.
"""
import math

import numpy as np

U = 2.0 ** -24
C_RESAMPLE, C_CONV, C_WARP = 8.0, 1.0, 10.0

# source length -> output length along the resampled axis
RATIOS = [
    (37, 5),    # strong down-sampling: 7.4 cells per output
    (50, 7),
    (23, 3),
    (65, 64),   # mild down-sampling: windows of one and two cells
    (40, 39),
    (25, 24),
    (19, 19),   # identity
    (17, 17),
    (64, 65),   # mild up-sampling
    (36, 37),
    (23, 25),
    (5, 37),    # strong up-sampling: windows of one cell (weight delta) and of two
    (3, 20),
    (1, 6),     # a single source cell
    (9, 1),     # a single output
]
RADII = [1, 2, 3, 6, 10, 25]


def asym_taps(radius):
    """2 R + 1 fixed float32 taps that are no palindrome: k[R - j] and k[R + j] give different results"""
    k = np.random.default_rng(7000 + radius).uniform(-1.0, 1.0, 2 * radius + 1).astype(np.float32)
    assert not np.array_equal(k, k[::-1])
    return k


# ---- definitions in binary64 ---------------------------------------------------------------------------------------------------------

def resample_weights(n, m):
    """[m, n] binary64: the share of source cell j in output i"""
    wt = np.zeros((m, n), np.float64)
    for i in range(m):
        for j in range(i * n // m, min(n, -((-(i + 1) * n) // m))):
            overlap = min((i + 1) * n, (j + 1) * m) - max(i * n, j * m)   # exact integers, in units of 1 / m
            wt[i, j] = overlap / n
    assert np.allclose(wt.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    return wt


def resample_axis(vol, m, axis):
    """vol [z, y, x] resampled to m cells along `axis` (0 = x, 1 = y, 2 = z as in the launchers)"""
    np_axis = 2 - axis
    v = np.moveaxis(np.asarray(vol, np.float64), np_axis, -1)
    out = v @ resample_weights(v.shape[-1], m).T
    return np.moveaxis(out, -1, np_axis)


def resample_bound(n, m, smax):
    return C_RESAMPLE * U * (m + math.ceil(n / m) + 1) * smax


def conv_axis(vol, taps, axis):
    np_axis = 2 - axis
    k = np.asarray(taps, np.float64)
    R = (len(k) - 1) // 2
    v = np.moveaxis(np.asarray(vol, np.float64), np_axis, -1)
    n = v.shape[-1]
    padded = np.zeros(v.shape[:-1] + (n + 2 * R,), np.float64)
    padded[..., R:R + n] = v
    out = np.zeros_like(v)
    for j in range(-R, R + 1):
        out += k[R - j] * padded[..., R + j:R + j + n]    # s[i + j]
    return np.moveaxis(out, -1, np_axis)


def conv_bound(taps, smax):
    R = (len(taps) - 1) // 2
    return C_CONV * U * (2 * R + 2) * float(np.abs(np.asarray(taps, np.float64)).sum()) * smax


def warp_coordinates(u, v, w, h):
    """(x_f, y_f, z_f, inside): the float32 sample coordinates of every voxel of dense [D, H, W] flows and the kernel's inside test"""
    D, H, W = u.shape
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        x_f = np.arange(W, dtype=np.float32)[None, None, :] + u * (one / np.float32(h[0]))
        y_f = np.arange(H, dtype=np.float32)[None, :, None] + v * (one / np.float32(h[1]))
        z_f = np.arange(D, dtype=np.float32)[:, None, None] + w * (one / np.float32(h[2]))
        outside = ((x_f < 0) | (x_f > np.float32(W - 1)) | (y_f < 0) | (y_f > np.float32(H - 1)) | (z_f < 0) | (z_f > np.float32(D - 1))
                   | np.isnan(x_f) | np.isnan(y_f) | np.isnan(z_f))
    assert x_f.dtype == y_f.dtype == z_f.dtype == np.float32
    return x_f, y_f, z_f, ~outside


def warp(f0, f1, u, v, w, h):
    """dense [D, H, W] float32 in, binary64 out"""
    D, H, W = f0.shape
    x_f, y_f, z_f, inside = warp_coordinates(u, v, w, h)
    out = np.asarray(f0, np.float64).copy()
    F = np.asarray(f1, np.float64)
    z, y, x = np.nonzero(inside)
    cx, cy, cz = (c[inside].astype(np.float64) for c in (x_f, y_f, z_f))
    x0, y0, z0 = (np.floor(c).astype(np.int64) for c in (cx, cy, cz))
    dx, dy, dz = cx - x0, cy - y0, cz - z0
    x1, y1, z1 = np.minimum(W - 1, x0 + 1), np.minimum(H - 1, y0 + 1), np.minimum(D - 1, z0 + 1)
    plane = lambda zz: ((1 - dx) * (1 - dy) * F[zz, y0, x0] + dx * (1 - dy) * F[zz, y0, x1] + (1 - dx) * dy * F[zz, y1, x0]
                        + dx * dy * F[zz, y1, x1])
    out[z, y, x] = (1 - dz) * plane(z0) + dz * plane(z1)
    return out


def warp_bound(f1max):
    return C_WARP * U * f1max


def worst(got, exact):
    """largest |got - exact|; a NaN anywhere counts as infinite"""
    d = np.abs(np.asarray(got, np.float64) - exact)
    return float("inf") if np.isnan(d).any() else float(d.max(initial=0.0))


# ---- shared warp inputs --------------------------------------------------------------------------------------------------------------

def flow_landing_on(target, spacing):
    """a float32 flow f with fl(f * fl(1 / spacing)) == target exactly, or None where no float32 gives it"""
    rcp = np.float32(1.0) / np.float32(spacing)
    t = np.float32(target)
    f = np.float32(t / rcp)
    for _ in range(4):
        f = np.nextafter(f, np.float32(-np.inf))
    for _ in range(9):
        if np.float32(f * rcp) == t:
            return f
        f = np.nextafter(f, np.float32(np.inf))
    return None


def planted_flows(n, spacing):
    """The edge landings of one axis of n cells: a list of (index, flow, expectation) with expectation "f0" (the voxel must receive
    frame_0), "in" (it must be interpolated) or None (whatever the oracle says)."""
    f32 = np.float32
    last = f32(n - 1)
    plant = [(n - 1, f32(0.0), "in"),                      # stays on the last cell: the min(n - 1, i + 1) clamp with fraction 0
             (0, f32(-0.0), "in"),                         # 0 + -0 = +0
             (0, f32(-1e-30), "f0"),                       # the smallest step below 0
             (n - 1, f32(np.spacing(last) * f32(spacing)) if n > 1 else f32(1e-30), "f0"),   # the float just above n - 1
             (n // 2, f32(np.inf), "f0"), (n // 2, f32(-np.inf), "f0"), (n // 2, f32(np.nan), "f0"), (n // 2, f32(-0.0), "in")]
    for t in range(1, n):                                  # a landing exactly on the last cell, and one exactly on 0, from t cells away
        f = flow_landing_on(t, spacing)
        if f is not None:
            plant += [(n - 1 - t, f, "in"), (t, f32(-f), "in")]
            break
    return plant


def warp_case(rng, dims, h, window=None, reach=2.9, plant=True):
    """Dense [D, H, W] float32 (f0, f1, u, v, w), the planted voxels [(z, y, x, expectation)] and the share of interpolated voxels of the
    random part.  window = (z_base, z_lo, z_hi, z_top): the planes [z_base, z_top) exist on the device and [z_lo, z_hi) are warped; w is
    made so that every voxel of the window reads f1 inside [z_base, z_top) only (asserted; see reads_stay_inside)."""
    W, H, D = dims
    z_base, z_lo, z_hi, z_top = window or (0, 0, D, D)
    f0 = rng.uniform(0, 255, (D, H, W)).astype(np.float32)
    f1 = rng.uniform(0, 255, (D, H, W)).astype(np.float32)
    u = rng.uniform(-0.6 * W * h[0], 0.6 * W * h[0], (D, H, W)).astype(np.float32)
    v = rng.uniform(-0.6 * H * h[1], 0.6 * H * h[1], (D, H, W)).astype(np.float32)
    w = rng.uniform(-reach * h[2], reach * h[2], (D, H, W)).astype(np.float32)
    if not plant:   # the smallest boxes: an axis of one cell is left by any flow but 0
        for a in (u, v, w):
            a[rng.random(a.shape) < 0.5] = 0.0
            a[rng.random(a.shape) < 0.1] = -0.0
    w[unsafe_reads(u, v, w, h, window)] = 0.0
    share = float(warp_coordinates(u, v, w, h)[3][z_lo:z_hi].mean())
    planted = []
    if plant:
        taken = set()

        def place(field, candidates, f, expect):
            """the first free voxel of `candidates` gets flow f in `field` and 0 in the other two components"""
            pos = next(p for p in candidates if p not in taken)
            taken.add(pos)
            for a in (u, v, w):
                a[pos] = 0.0
            field[pos] = f
            planted.append(pos + (expect,))

        for i, f, expect in planted_flows(W, h[0]):
            place(u, ((z, y, i) for z in range(z_lo, z_hi) for y in range(H)), f, expect)
        for i, f, expect in planted_flows(H, h[1]):
            place(v, ((z, i, x) for z in range(z_lo, z_hi) for x in range(W)), f, expect)
        for i, f, expect in planted_flows(D, h[2]):
            if z_lo <= i < z_hi:                           # (the windows of the tests hold plane 0 and plane D - 1 between them)
                place(w, ((i, y, x) for y in range(H) for x in range(W)), f, expect)
    assert not unsafe_reads(u, v, w, h, window).any()
    return (f0, f1, u, v, w), planted, share


def unsafe_reads(u, v, w, h, window):
    """[D, H, W] bool: voxels of the window whose sample would read a plane of frame_1 outside [z_base, z_top).  Judged on z alone (as if
    x and y were always inside), with the kernel's own float32 z_f: floor(z_f) and min(D - 1, floor(z_f) + 1) must both be held."""
    D = u.shape[0]
    z_base, z_lo, z_hi, z_top = window or (0, 0, D, D)
    z_f = warp_coordinates(u, v, w, h)[2]
    with np.errstate(invalid="ignore"):
        reads = (z_f >= 0) & (z_f <= np.float32(D - 1))
        lo = np.floor(np.where(reads, z_f, 0)).astype(np.int64)
    hi = np.minimum(D - 1, lo + 1)
    bad = reads & ((lo < z_base) | (hi > z_top - 1))
    bad[:z_lo] = False
    bad[z_hi:] = False
    return bad
