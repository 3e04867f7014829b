"""Numpy restatement of the strain fields over a strain window (include/f3d.h, f3d_window_strain), the checker of the kernel.

d = (u, v, w) on a [z, y, x] grid.  A grid point is present when it lies inside the volume and none of its components is NaN.  The
volume is padded by r absent points on every side; over the (2r+1)^3 window of every voxel
    the mask moments n, Sx .. Szz are int64 sums of shifted slices,
    the data sums are float64 sums of shifted slices, x then y then z, every sum started with its first term and added in ascending
        offset, every product by the float64 offset formed on its own (t = +0 at an absent point),
    the normal matrix, its adjugate and determinant are int64, the right-hand side and the solution float64 with one division per
        entry of G, rounded to float32,
and the eight strain fields come from G through strain_ref.fields_of_gradient.  Only exact integers, order-fixed IEEE binary64
+ - * / and that float32 tail take part, so this agrees with the kernel bit for bit (NaN positions, not payloads)."""
import numpy as np

from strain_ref import NAMES as STRAIN_NAMES, fields_of_gradient, same_bits  # noqa: F401  (same_bits: for the tests)

F32, F64, I64 = np.float32, np.float64, np.int64
GRAD_NAMES = ("G00", "G01", "G02", "G10", "G11", "G12", "G20", "G21", "G22")
NAMES = STRAIN_NAMES + GRAD_NAMES
GROUP_OF = (1, 2, 2, 2, 2, 2, 2, 4) + (8,) * 9


def default_min_count(radius):
    return max(4, (2 * radius + 1) ** 3 // 4)


def _wsum(a, axis, r, power=0):
    """the 'valid' window sum along `axis` of an array that carries r extra points at either end of it:
    (((o^power a[p - r]) + (o^power a[p - r + 1])) + ...) for o = -r .. r (power 0: no product at all)"""
    n = a.shape[axis] - 2 * r
    acc = None
    for o in range(-r, r + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(o + r, o + r + n)
        term = a[tuple(sl)]
        if power:
            term = a.dtype.type(o ** power) * term
        acc = term if acc is None else acc + term
    return acc


def moments(present, r):
    """dict of the ten int64 mask moments of every voxel"""
    m = np.pad(present.astype(I64), r)
    X, Y, Z = 2, 1, 0
    nx, sx, sxx = _wsum(m, X, r), _wsum(m, X, r, 1), _wsum(m, X, r, 2)
    n_xy, sx_xy, sxx_xy = _wsum(nx, Y, r), _wsum(sx, Y, r), _wsum(sxx, Y, r)
    sy_xy, sxy_xy, syy_xy = _wsum(nx, Y, r, 1), _wsum(sx, Y, r, 1), _wsum(nx, Y, r, 2)
    return {"n": _wsum(n_xy, Z, r), "Sx": _wsum(sx_xy, Z, r), "Sy": _wsum(sy_xy, Z, r), "Sz": _wsum(n_xy, Z, r, 1),
            "Sxx": _wsum(sxx_xy, Z, r), "Sxy": _wsum(sxy_xy, Z, r), "Sxz": _wsum(sx_xy, Z, r, 1), "Syy": _wsum(syy_xy, Z, r),
            "Syz": _wsum(sy_xy, Z, r, 1), "Szz": _wsum(n_xy, Z, r, 2)}


def data_sums(comp, present, r):
    """(D0, Dx, Dy, Dz) of one component, float64"""
    t = np.pad(np.where(present, comp.astype(F64), F64(0)), r)
    X, Y, Z = 2, 1, 0
    a0, a1 = _wsum(t, X, r), _wsum(t, X, r, 1)
    b00, b10, b01 = _wsum(a0, Y, r), _wsum(a1, Y, r), _wsum(a0, Y, r, 1)
    return _wsum(b00, Z, r), _wsum(b10, Z, r), _wsum(b01, Z, r), _wsum(b00, Z, r, 1)


def window_gradient(u, v, w, radius, min_count=None):
    """(G, present, fitted): G[c][a] float32 arrays (garbage where not fitted), the presence of every voxel, and where the fit exists"""
    r = int(radius)
    assert 1 <= r <= 3
    k = default_min_count(r) if min_count is None else int(min_count)
    assert 1 <= k <= (2 * r + 1) ** 3
    d = [np.asarray(a, dtype=F32) for a in (u, v, w)]
    depth, height, width = d[0].shape
    present = ~(np.isnan(d[0]) | np.isnan(d[1]) | np.isnan(d[2]))
    M = moments(present, r)
    n, S = M["n"], (M["Sx"], M["Sy"], M["Sz"])
    c00 = n * M["Sxx"] - S[0] * S[0] if width > 1 else np.ones_like(n)
    c11 = n * M["Syy"] - S[1] * S[1] if height > 1 else np.ones_like(n)
    c22 = n * M["Szz"] - S[2] * S[2] if depth > 1 else np.ones_like(n)
    c01, c02, c12 = n * M["Sxy"] - S[0] * S[1], n * M["Sxz"] - S[0] * S[2], n * M["Syz"] - S[1] * S[2]
    adj = [[c11 * c22 - c12 * c12, c02 * c12 - c01 * c22, c01 * c12 - c02 * c11],
           [None, c00 * c22 - c02 * c02, c01 * c02 - c00 * c12],
           [None, None, c00 * c11 - c01 * c01]]
    adj[1][0], adj[2][0], adj[2][1] = adj[0][1], adj[0][2], adj[1][2]
    det = c00 * adj[0][0] + c01 * adj[1][0] + c02 * adj[2][0]
    fitted = present & (n >= k) & (det != 0)
    dn, dS, ddet = n.astype(F64), [s.astype(F64) for s in S], det.astype(F64)
    dadj = [[a.astype(F64) for a in row] for row in adj]
    G = [[None] * 3 for _ in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in range(3):
            D0, Dx, Dy, Dz = data_sums(d[c], present, r)
            rhs = [dn * Dx - dS[0] * D0, dn * Dy - dS[1] * D0, dn * Dz - dS[2] * D0]
            for a in range(3):
                num = (dadj[a][0] * rhs[0] + dadj[a][1] * rhs[1]) + dadj[a][2] * rhs[2]
                G[c][a] = (num / ddet).astype(F32)
    return G, present, fitted


def window_strain_ref(u, v, w, radius, min_count=None):
    """(fields, stats): dict name -> float32 [z, y, x] array of all seventeen outputs (NaN where the voxel is undefined), and the
    statistics of f3d_window_strain (vol_sum in float64 in numpy's order; vol_abs_sum scales its tolerance)"""
    G, present, fitted = window_gradient(u, v, w, radius, min_count)
    nan = F32(np.nan)
    G = [[np.where(fitted, G[c][a], nan).astype(F32) for a in range(3)] for c in range(3)]
    out = fields_of_gradient(G)
    for c in range(3):
        for a in range(3):
            out[f"G{c}{a}"] = G[c][a]
    vol, eq = out["vol"], out["eq"]
    ok = ~np.isnan(vol)
    count = int(ok.sum())
    fnan = float("nan")
    stats = {"defined": count, "folded": int((vol[ok] <= F32(-1)).sum()), "lost": int((~present).sum()),
             "thin": int((present & ~fitted).sum()),
             "vol_min": float(vol[ok].min()) if count else fnan, "vol_max": float(vol[ok].max()) if count else fnan,
             "eq_max": float(eq[ok].max()) if count else fnan, "vol_sum": float(vol[ok].astype(F64).sum()),
             "vol_abs_sum": float(np.abs(vol[ok].astype(F64)).sum())}
    return out, stats
