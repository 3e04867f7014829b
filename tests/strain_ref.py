"""Float32 numpy restatement of the strain fields of a displacement (include/f3d.h, f3d_flow_strain), the checker of the kernel.

d = (u, v, w) on a [z, y, x] grid, voxel units.  G[r][c] = d d_r / d x_c (row r = component u, v, w; column c = axis x, y, z).
A grid point is missing when it lies outside the volume or any of its components is NaN.  Per voxel p and axis a of size n:
    p missing                  -> every output NaN
    n == 1                     -> column a of G is 0
    m = p - e_a, q = p + e_a:  both present: (d(q) - d(m)) * 0.5;  only q: d(q) - d(p);  only m: d(p) - d(m);  neither: all NaN
The outputs are formed from G in include/f3d.h's order, every operation rounded to float32 on its own, so this agrees with the
kernel bit for bit (NaN positions, not payloads)."""
import numpy as np

F32 = np.float32
NAMES = ("vol", "exx", "eyy", "ezz", "exy", "exz", "eyz", "eq")
GROUP = {"vol": "vol", "exx": "e", "eyy": "e", "ezz": "e", "exy": "e", "exz": "e", "eyz": "e", "eq": "eq"}


def _shift(a, axis, s):
    """the value at p + s * e_axis (NaN outside the volume)"""
    out = np.full_like(a, np.nan)
    n = a.shape[axis]
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if s > 0:
        src[axis], dst[axis] = slice(1, n), slice(0, n - 1)
    else:
        src[axis], dst[axis] = slice(0, n - 1), slice(1, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _present(comps):
    return ~(np.isnan(comps[0]) | np.isnan(comps[1]) | np.isnan(comps[2]))


def gradient_ref(u, v, w):
    """(G, defined): G[r][c] float32 arrays and the voxels where every column exists and p is present"""
    d = [np.asarray(a, dtype=F32) for a in (u, v, w)]
    here = _present(d)
    defined = here.copy()
    G = [[None] * 3 for _ in range(3)]
    half = F32(0.5)
    for c, axis in enumerate((2, 1, 0)):                 # x, y, z = numpy axes 2, 1, 0
        if d[0].shape[axis] == 1:
            for r in range(3):
                G[r][c] = np.zeros_like(d[0])
            continue
        m = [_shift(a, axis, -1) for a in d]
        q = [_shift(a, axis, +1) for a in d]
        hm, hq = _present(m), _present(q)
        with np.errstate(invalid="ignore"):
            for r in range(3):
                G[r][c] = np.where(hm & hq, (q[r] - m[r]) * half,
                                   np.where(hq, q[r] - d[r], np.where(hm, d[r] - m[r], F32(np.nan)))).astype(F32)
        defined &= hm | hq
    return G, defined


def fields_of_gradient(G):
    """the eight outputs (dict name -> float32 array) of a gradient, in include/f3d.h's evaluation order"""
    G00, G01, G02 = G[0]
    G10, G11, G12 = G[1]
    G20, G21, G22 = G[2]
    with np.errstate(invalid="ignore", over="ignore"):
        I1 = (G00 + G11) + G22
        I2 = ((G00 * G11 - G01 * G10) + (G11 * G22 - G12 * G21)) + (G00 * G22 - G02 * G20)
        I3 = (G00 * (G11 * G22 - G12 * G21) - G01 * (G10 * G22 - G12 * G20)) + G02 * (G10 * G21 - G11 * G20)
        vol = (I1 + I2) + I3
        half = F32(0.5)

        def e(r, c):
            return half * ((G[r][c] + G[c][r]) + ((G[0][r] * G[0][c] + G[1][r] * G[1][c]) + G[2][r] * G[2][c]))

        exx, eyy, ezz, exy, exz, eyz = e(0, 0), e(1, 1), e(2, 2), e(0, 1), e(0, 2), e(1, 2)
        m = ((exx + eyy) + ezz) / F32(3)
        a, b, c = exx - m, eyy - m, ezz - m
        s = ((a * a + b * b) + c * c) + F32(2) * ((exy * exy + exz * exz) + eyz * eyz)
        eq = np.sqrt(s / F32(1.5))
    out = dict(zip(NAMES, (vol, exx, eyy, ezz, exy, exz, eyz, eq)))
    return {k: np.asarray(x, dtype=F32) for k, x in out.items()}


def strain_ref(u, v, w):
    """dict name -> float32 [z, y, x] array of all eight outputs (NaN where the voxel is undefined)"""
    G, defined = gradient_ref(u, v, w)
    out = fields_of_gradient(G)
    for k in out:
        out[k] = np.where(defined, out[k], F32(np.nan)).astype(F32)
    return out


def strain_stats_ref(vol, eq):
    """the statistics of f3d_flow_strain from the restatement's vol and eq (vol_sum in float64, summation order numpy's)"""
    ok = ~np.isnan(vol)
    n = int(ok.sum())
    nan = float("nan")
    return {
        "defined": n,
        "folded": int((vol[ok] <= F32(-1)).sum()),
        "vol_min": float(vol[ok].min()) if n else nan,
        "vol_max": float(vol[ok].max()) if n else nan,
        "eq_max": float(eq[ok].max()) if n else nan,
        "vol_sum": float(vol[ok].astype(np.float64).sum()),
    }


def same_bits(a, b):
    """equal as float32 values with NaN at the same positions (payloads not compared)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
