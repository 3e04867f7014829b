"""Independent references for the device kernels that have no counterpart in the reference code (f3d_flow_strain, f3d_compose_flow,
f3d_abs_max, f3d_flow_stats, f3d_residual_stats), written from include/f3d.h and not from tests/strain_ref.py or
tests/trajectory_ref.py:

  * exact constructions: affine displacements and flows on integer grids with dyadic coefficients of few bits, for which every float32
    operation of include/f3d.h's evaluation order is exact.  The helpers prove that exactness themselves (dyadic bounds and float64
    error-free transformations), so the kernel must return the closed form itself;
  * a float64 strain of the header's definition: np.gradient (central inside, one-sided at faces) on hole-free volumes, a masked
    float64 stencil where there are NaN holes, and det / Green-Lagrange / von Mises from their definitions, with a tolerance derived
    from float32 rounding of the stated expressions;
  * exact sums (math.fsum) and scans for the statistics."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
F64 = np.float64
EPS32 = 2.0 ** -24           # unit roundoff of float32
NAMES = ("vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq")


# ---- exactness proofs ---------------------------------------------------------------------------------------------------------

def f32_exact(x):
    """True when every value of x (float64, NaN ignored) is a float32"""
    x = np.asarray(x, F64)
    ok = ~np.isnan(x)
    return bool(np.array_equal(x[ok].astype(F32).astype(F64), x[ok]))


def exact_add(a, b):
    """a + b in float64, asserting that the sum is exact (TwoSum error term 0) and a float32: so float32 rounds it to itself"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    assert np.all(err[np.isfinite(err)] == 0), "a float32 sum of the construction is not exact"
    assert f32_exact(s), "a sum of the construction is not a float32"
    return s


def exact_mul(a, b):
    """a * b of float32 values: exact in float64 (48 significant bits); asserted to be a float32"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert f32_exact(a) and f32_exact(b)
    p = a * b
    assert f32_exact(p), "a float32 product of the construction is not exact"
    return p


def granularity(values):
    """the smallest q >= 0 such that every value is an integer multiple of 2^-q (at most 60)"""
    vals = [Fraction(v) for v in np.ravel(values)]
    q = 0
    while any((v * 2 ** q).denominator != 1 for v in vals):
        q += 1
        assert q <= 60
    return q


# ---- strain of an affine displacement -----------------------------------------------------------------------------------------

def affine_field(A, b, dims, z0=0, z1=None):
    """d_r = A[r] . (x, y, z) + b[r] on planes [z0, z1) of a W x H x D grid, float32 [z, y, x] per component, built by float32 adds
    of per-axis terms.  Exact (asserted): every coefficient is dyadic and every term and partial sum a float32."""
    w, h, d = dims
    z1 = d if z1 is None else z1
    x, y, z = np.arange(w, dtype=F64), np.arange(h, dtype=F64), np.arange(z0, z1, dtype=F64)
    out = []
    for r in range(3):
        tx, ty, tz = A[r][0] * x, A[r][1] * y, A[r][2] * z + b[r]
        bound = np.abs(tx).max() + np.abs(ty).max() + np.abs(tz).max()
        q = max(granularity([A[r][c] for c in range(3)] + [b[r]]), 0)
        assert bound * 2.0 ** q < 2.0 ** 24, "affine field too large for exact float32"
        assert f32_exact(tx) and f32_exact(ty) and f32_exact(tz)
        out.append((tz.astype(F32)[:, None, None] + ty.astype(F32)[None, :, None]) + tx.astype(F32)[None, None, :])
    return out


def header_fields_exact(G):
    """vol and the six E components of a constant gradient G (3 x 3 floats) evaluated in include/f3d.h's order with every float32
    operation proven exact (so the float32 result is the exact value); returns dict name -> float"""
    g = [[F64(G[r][c]) for c in range(3)] for r in range(3)]
    assert all(f32_exact(g[r][c]) for r in range(3) for c in range(3))
    add, mul = exact_add, exact_mul
    sub = lambda a, b: exact_add(a, -np.asarray(b, F64))
    G00, G01, G02 = g[0]
    G10, G11, G12 = g[1]
    G20, G21, G22 = g[2]
    I1 = add(add(G00, G11), G22)
    I2 = add(add(sub(mul(G00, G11), mul(G01, G10)), sub(mul(G11, G22), mul(G12, G21))), sub(mul(G00, G22), mul(G02, G20)))
    I3 = add(sub(mul(G00, sub(mul(G11, G22), mul(G12, G21))), mul(G01, sub(mul(G10, G22), mul(G12, G20)))),
             mul(G02, sub(mul(G10, G21), mul(G11, G20))))
    out = {"vol": float(add(add(I1, I2), I3))}

    def e(r, c):
        return float(mul(0.5, add(add(g[r][c], g[c][r]), add(add(mul(g[0][r], g[0][c]), mul(g[1][r], g[1][c])), mul(g[2][r], g[2][c])))))

    for n, (r, c) in zip(NAMES[1:7], ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[n] = e(r, c)
    return out


def closed_form_fraction(A):
    """exact vol = det(I + A) - 1 and E = 1/2 (A + A^T + A^T A) of a dyadic matrix, as Fractions"""
    a = [[Fraction(A[r][c]) for c in range(3)] for r in range(3)]
    F = [[a[r][c] + (1 if r == c else 0) for c in range(3)] for r in range(3)]
    det = (F[0][0] * (F[1][1] * F[2][2] - F[1][2] * F[2][1]) - F[0][1] * (F[1][0] * F[2][2] - F[1][2] * F[2][0]) +
           F[0][2] * (F[1][0] * F[2][1] - F[1][1] * F[2][0]))
    E = lambda r, c: (a[r][c] + a[c][r] + sum(a[k][r] * a[k][c] for k in range(3))) / 2
    out = {"vol": det - 1}
    for n, (r, c) in zip(NAMES[1:7], ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[n] = E(r, c)
    return out


def eq_of_E(E):
    """float64 von Mises equivalent strain sqrt(2/3 dev(E) : dev(E)) of a dict or of arrays exx .. eyz"""
    exx, eyy, ezz, exy, exz, eyz = (np.asarray(E[n], F64) for n in NAMES[1:7])
    m = (exx + eyy + ezz) / 3
    s = (exx - m) ** 2 + (eyy - m) ** 2 + (ezz - m) ** 2 + 2 * (exy ** 2 + exz ** 2 + eyz ** 2)
    return np.sqrt(s * (2.0 / 3.0))


EQ_ULPS = 8   # eq = sqrtf(s / 1.5f) after a division by 3, three subtractions, eight products and sums: a few roundings


def ulps_apart(a, b):
    """|a - b| in float32 ulps of b (a, b float64 scalars or arrays)"""
    b32 = np.asarray(b, F32)
    return np.abs(np.asarray(a, F64) - np.asarray(b, F64)) / np.spacing(np.abs(b32)).astype(F64)


def missing_mask(u, v, w):
    return np.isnan(u) | np.isnan(v) | np.isnan(w)


def predicted_undefined(missing):
    """the voxels f3d_flow_strain leaves NaN, from the missing set alone (include/f3d.h): the voxel is missing, or along some axis of
    size > 1 neither neighbour is present (outside the volume counts as missing)"""
    und = missing.copy()
    for axis in range(3):
        n = missing.shape[axis]
        if n == 1:
            continue
        has_m = np.zeros_like(missing)
        has_q = np.zeros_like(missing)
        sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(3))
        has_m[sl(1, n)] = ~missing[sl(0, n - 1)]
        has_q[sl(0, n - 1)] = ~missing[sl(1, n)]
        und |= ~(has_m | has_q)
    return und


# ---- float64 strain from the header's definition ---------------------------------------------------------------------------

def gradient64(u, v, w):
    """float64 G[r][c] of a displacement (NaN marks missing samples): the header's rule as a masked stencil.  On a hole-free volume it
    is np.gradient(edge_order=1) per axis (the CPU tests check that)."""
    comps = [np.asarray(a, F64) for a in (u, v, w)]
    miss = missing_mask(*comps)
    G = [[None] * 3 for _ in range(3)]
    undefined = miss.copy()
    for c, axis in enumerate((2, 1, 0)):
        n = miss.shape[axis]
        if n == 1:
            for r in range(3):
                G[r][c] = np.zeros(miss.shape)
            continue
        sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(3))
        has_m = np.zeros_like(miss)
        has_q = np.zeros_like(miss)
        has_m[sl(1, n)] = ~miss[sl(0, n - 1)]
        has_q[sl(0, n - 1)] = ~miss[sl(1, n)]
        undefined |= ~(has_m | has_q)
        for r in range(3):
            f = comps[r]
            fm = np.full(f.shape, np.nan)
            fq = np.full(f.shape, np.nan)
            fm[sl(1, n)] = f[sl(0, n - 1)]
            fq[sl(0, n - 1)] = f[sl(1, n)]
            with np.errstate(invalid="ignore"):
                G[r][c] = np.where(has_m & has_q, (fq - fm) / 2, np.where(has_q, fq - f, np.where(has_m, f - fm, np.nan)))
    return G, undefined


def gradient_np(u, v, w):
    """float64 G of a hole-free displacement with np.gradient(edge_order=1): central inside, one-sided at faces, 0 on size-1 axes"""
    G = [[None] * 3 for _ in range(3)]
    for r, comp in enumerate((u, v, w)):
        f = np.asarray(comp, F64)
        for c, axis in enumerate((2, 1, 0)):
            G[r][c] = np.gradient(f, axis=axis, edge_order=1) if f.shape[axis] > 1 else np.zeros(f.shape)
    return G


def strain64(G, undefined=None):
    """float64 vol = det(I + G) - 1, E = 1/2 (F^T F - I), eq = sqrt(2/3 dev E : dev E); NaN where undefined"""
    Gm = np.stack([np.stack(G[r], axis=-1) for r in range(3)], axis=-2)       # [..., r, c]
    bad = np.isnan(Gm).any(axis=(-1, -2))
    if undefined is not None:
        bad = bad | undefined
    Gm = np.where(bad[..., None, None], 0.0, Gm)
    F = Gm + np.eye(3)
    vol = np.linalg.det(F) - 1
    E = 0.5 * (np.swapaxes(F, -1, -2) @ F - np.eye(3))
    out = {"vol": vol}
    for n, (r, c) in zip(NAMES[1:7], ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[n] = E[..., r, c]
    out["eq"] = eq_of_E(out)
    for k in out:
        out[k] = np.where(bad, np.nan, out[k])
    return out


def strain_tolerance(G):
    """per-voxel bounds on |float32 kernel - float64 header| for vol, the E components and eq^2.

    The kernel sees float32 samples (the float64 reference is fed the same values), so the only errors are float32 roundings: the
    gradient itself (one rounding per difference and one per halving, relative 2^-24 each) and the roundings of the stated
    expressions.  With g = max |G| each term of vol is at most (1 + g)^3 in size and each of E or s at most (1 + g)^2 resp.
    (1 + g)^4; twenty roundings of terms that size bound the sum.  The bound is far below the change that a wrong neighbour or a
    wrong side makes to a non-affine field (order of the second derivative)."""
    g = np.max(np.stack([np.abs(G[r][c]) for r in range(3) for c in range(3)]), axis=0)
    g = np.where(np.isnan(g), 0.0, g)
    k = 32 * EPS32
    return {"vol": k * (1 + g) ** 3, "e": k * (1 + g) ** 2, "eq2": k * (1 + g) ** 4}


def smooth_displacement(dims, kind, amp=0.05, seed=0):
    """a non-affine float32 displacement whose central and one-sided differences differ clearly: "quadratic" (a dyadic quadratic
    form of the centred coordinates) or "sine" (products of sinusoids of a few voxels' wavelength)"""
    w, h, d = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(d, dtype=F64), np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    p = [(x - (w - 1) / 2) / max(w, 2), (y - (h - 1) / 2) / max(h, 2), (z - (d - 1) / 2) / max(d, 2)]
    out = []
    for r in range(3):
        if kind == "quadratic":
            c = rng.integers(-8, 9, size=(3, 3))
            f = sum(c[i][j] * p[i] * p[j] * max(w, h, d) for i in range(3) for j in range(3)) * amp
        else:
            k = rng.uniform(0.3, 0.9, size=3)
            f = amp * 3 * np.sin(k[0] * x + r) * np.cos(k[1] * y - r) * np.sin(k[2] * z + 0.5)
        out.append(f.astype(F32))
    return out


# ---- composition of affine flows ----------------------------------------------------------------------------------------

def affine_compose_coeffs(steps):
    """exact (Fraction) coefficients (C, c) of the displacement after each step, starting from zero: a_k(x) = a_{k-1}(x) + A_k (x +
    a_{k-1}(x)) + b_k, i.e. C_k = C + A (I + C), c_k = c + A c + b; steps = [(A, b), ...]"""
    C = [[Fraction(0)] * 3 for _ in range(3)]
    c = [Fraction(0)] * 3
    out = []
    for A, b in steps:
        A = [[Fraction(A[r][k]) for k in range(3)] for r in range(3)]
        b = [Fraction(x) for x in b]
        IC = [[C[r][k] + (1 if r == k else 0) for k in range(3)] for r in range(3)]
        C = [[C[r][k] + sum(A[r][j] * IC[j][k] for j in range(3)) for k in range(3)] for r in range(3)]
        c = [c[r] + sum(A[r][j] * c[j] for j in range(3)) + b[r] for r in range(3)]
        out.append((C, c))
    return out


def prove_compose_exact(steps, dims):
    """assert that every float32 operation of f3d_compose_flow is exact for the affine steps on a W x H x D grid (dyadic bounds on
    the operation sequence of the header / k_warp's trilinear sample), so that each step returns acc + inc(x + acc) exactly; a point
    lies inside or outside by its exact position"""
    w, h, d = dims
    ext = [w - 1, h - 1, d - 1]
    accs = [([[Fraction(0)] * 3 for _ in range(3)], [Fraction(0)] * 3)] + affine_compose_coeffs(steps)[:-1]
    for (A, b), (C, c) in zip(steps, accs):
        A = [[Fraction(v) for v in row] for row in A]
        b = [Fraction(v) for v in b]
        q_acc = max(granularity([C[r][k] for r in range(3) for k in range(3)] + list(c)), 0)
        # |acc| and |inc| over the grid, and the granularity of inc at grid points
        acc_max = max(sum(abs(C[r][k]) * ext[k] for k in range(3)) + abs(c[r]) for r in range(3))
        inc_max = max(sum(abs(A[r][k]) * ext[k] for k in range(3)) + abs(b[r]) for r in range(3))
        q_inc = max(granularity([A[r][k] for r in range(3) for k in range(3)] + list(b)), 0)
        # p = x + acc: granularity q_acc; weights 1 - t and t in [0, 1], granularity q_acc; weight products 2 q_acc and 3 q_acc;
        # every partial sum of the sample is at most inc_max (non-negative weights of sum <= 1); the update acc + sample
        assert (max(ext) + acc_max) * 2 ** q_acc < 2 ** 24, "position not exact"
        assert inc_max * 2 ** (3 * q_acc + q_inc) < 2 ** 24, "trilinear sample not exact"
        assert (acc_max + inc_max) * 2 ** max(q_acc, 3 * q_acc + q_inc) < 2 ** 24, "update not exact"
        assert inc_max * 2 ** q_inc < 2 ** 24
    return True


def affine_eval(C, c, dims, z0=0, z1=None):
    """float32 [z, y, x] components of C x + c on planes [z0, z1) (exact: asserted through affine_field)"""
    return affine_field([[float(v) for v in row] for row in C], [float(v) for v in c], dims, z0, z1)


def compose_affine_expected(steps, dims, z0=0, z1=None):
    """the exact displacement after every step of `steps` on planes [z0, z1): a list of (u, v, w) float32 with NaN where the point
    has left [0, n-1] at this step or before"""
    w, h, d = dims
    z1 = d if z1 is None else z1
    coeffs = affine_compose_coeffs(steps)
    prev = None
    lost = None
    out = []
    zz, yy, xx = np.meshgrid(np.arange(z0, z1, dtype=F64), np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    for k, (C, c) in enumerate(coeffs):
        a_prev = [np.zeros(xx.shape)] * 3 if prev is None else [a.astype(F64) for a in prev]
        pos = (xx + a_prev[0], yy + a_prev[1], zz + a_prev[2])
        outside = np.zeros(xx.shape, bool)
        for p, n in zip(pos, (w, h, d)):
            outside |= (p < 0) | (p > n - 1)
        lost = outside if lost is None else (lost | outside)
        cur = affine_eval(C, c, dims, z0, z1)
        prev = [np.where(lost, np.nan, a).astype(F32) for a in cur]
        out.append(tuple(prev))
    return out


# ---- statistics -------------------------------------------------------------------------------------------------------------

def fsum(values):
    """exact (correctly rounded) float64 sum of float64 values"""
    return math.fsum(np.asarray(values, F64).ravel().tolist())


def magnitude32(u, v, w):
    """|(u, v, w)| as k_flow_stats forms it: sqrtf((a*a + b*b) + c*c) in float32"""
    u, v, w = (np.asarray(a, F32) for a in (u, v, w))
    return np.sqrt((u * u + v * v) + w * w)


def finite_abs_max(a):
    """the largest finite |x| (0 when there is none): f3d_abs_max's contract"""
    a = np.abs(np.asarray(a, F32))
    a = a[np.isfinite(a)]
    return F32(a.max()) if a.size else F32(0)


# ---- holes ----------------------------------------------------------------------------------------------------------------

def seam_holes(dims, rng, density=0.01):
    """(all_nan, one_nan) masks [z, y, x]: single missing voxels and short runs on the seams of the strain kernel's tiling (x = 62..65
    and 126..129, y = 3 / 4, z = 30..33 and 62..65) and on every face, plus a sprinkle of random ones.  all_nan voxels lose all three
    components, one_nan voxels only one (enough to make the point missing)."""
    w, h, d = dims
    all_nan = rng.random((d, h, w)) < density
    one_nan = rng.random((d, h, w)) < density / 2
    seams = lambda n, cuts: [c for c in cuts if c < n]
    for x in seams(w, (62, 63, 64, 65, 126, 127, 128, 129)):
        sel = rng.random((d, h)) < 0.3
        all_nan[:, :, x] |= sel
    for y in seams(h, (3, 4)):
        all_nan[:, y, :] |= rng.random((d, w)) < 0.3
    for z in seams(d, (30, 31, 32, 33, 62, 63, 64, 65)):
        all_nan[z] |= rng.random((h, w)) < 0.3
    faces = []
    if w > 1:
        faces += [(slice(None), slice(None), 0), (slice(None), slice(None), w - 1)]
    if h > 1:
        faces += [(slice(None), 0, slice(None)), (slice(None), h - 1, slice(None))]
    if d > 1:
        faces += [(0, slice(None), slice(None)), (d - 1, slice(None), slice(None))]
    for face in faces:           # an axis of size one has no face of its own: its "face" is the whole volume
        sub = all_nan[face]
        all_nan[face] = sub | (rng.random(sub.shape) < 0.2)
        sub = one_nan[face]
        one_nan[face] = sub | (rng.random(sub.shape) < 0.05)
    return all_nan, one_nan & ~all_nan


def with_holes(comps, all_nan, one_nan, which=1):
    """copies of the components with all_nan voxels NaN in every component and one_nan voxels NaN in component `which`"""
    out = [np.array(c, dtype=F32) for c in comps]
    for c in out:
        c[all_nan] = np.nan
    out[which][one_nan] = np.nan
    return out


# ---- the constructions the tests share ------------------------------------------------------------------------------------

# constant gradients of affine displacements (dyadic, few bits): a mild general one and a strong compression with shear
STRAIN_AFFINE = (
    ([[3 / 32, -5 / 64, 1 / 16], [1 / 32, -7 / 64, 3 / 64], [-1 / 16, 1 / 64, 5 / 32]], [1 / 4, -3 / 8, 1 / 2]),
    ([[-1 / 2, 1 / 4, 0], [1 / 8, -3 / 4, 1 / 8], [0, 1 / 4, -5 / 8]], [-2, 1 / 2, 3]),
)

# affine flows of successive pairs, composed from zero: expansion / shear that sends points out through several faces
COMPOSE_AFFINE = (
    ([[1 / 8, 0, -1 / 8], [1 / 8, -1 / 8, 0], [0, 1 / 8, 1 / 8]], [1 / 2, -3 / 8, 1 / 4]),
    ([[-1 / 4, 1 / 4, 0], [0, 1 / 4, -1 / 4], [1 / 4, 0, -1 / 4]], [-1, 1 / 2, 3 / 4]),
    ([[1 / 4, 0, 0], [0, -1 / 4, 0], [0, 0, 1 / 4]], [1 / 2, -1 / 2, 1 / 4]),
)
