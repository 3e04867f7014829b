"""numpy restatement of the motion fit of include/f3d.h and include/f3d_host.h, written from the headers: the presence rule and the
moment sums of f3d_motion_sums (the coordinate sums as Python integers of doubled coordinates, the displacement sums by math.fsum of
the binary64 terms), the expression of f3d_remove_motion in float64 numpy in the stated order, and the fits by numpy's own
least squares (affine) and singular value decomposition (Kabsch) from the voxels themselves, not from the sums.  At the end, the
fields the tests construct: an affine displacement about the centre, a seeded hole mask, a rotation matrix."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
F64 = np.float64
SXX_ORDER = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # xx yy zz xy xz yz


def present_mask(u, v, w, weight=None, weight_min=0.8):
    m = ~(np.isnan(u) | np.isnan(v) | np.isnan(w))
    if weight is not None:
        with np.errstate(invalid="ignore"):
            m &= weight >= F32(weight_min)          # a NaN weight fails the comparison
    return m


def doubled_coordinates(shape):
    """2x - (W-1), 2y - (H-1), 2z - (D-1) as int64 volumes [z, y, x]"""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d, dtype=np.int64), np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return 2 * x - (w - 1), 2 * y - (h - 1), 2 * z - (d - 1)


def motion_sums(u, v, w, weight=None, weight_min=0.8):
    """dict: n, x2[3], xx4[6] (exact Python integers of doubled coordinates), Sx, Sxx (those as floats, exactly when representable),
    Sd, Sxd, Sdd (math.fsum of the binary64 terms) and, for the bound of any summation order, abs_d, abs_xd, abs_dd = sum |term|"""
    m = present_mask(u, v, w, weight, weight_min)
    c2 = [c[m] for c in doubled_coordinates(u.shape)]
    d = [a[m].astype(F64) for a in (u, v, w)]
    X = [c.astype(F64) * 0.5 for c in c2]                        # half-integers, exact
    out = {"n": int(m.sum())}
    out["x2"] = [int(c.sum()) for c in c2]
    out["xx4"] = [int((c2[i] * c2[k]).sum()) for i, k in SXX_ORDER]
    out["Sx"] = [float(Fraction(s, 2)) for s in out["x2"]]
    out["Sxx"] = [float(Fraction(s, 4)) for s in out["xx4"]]
    out["Sd"] = [math.fsum(a) for a in d]
    out["abs_d"] = [math.fsum(np.abs(a)) for a in d]
    out["Sxd"], out["abs_xd"] = [], []
    for i in range(3):
        for j in range(3):
            term = X[i] * d[j]                                   # one rounding per term
            out["Sxd"].append(math.fsum(term))
            out["abs_xd"].append(math.fsum(np.abs(term)))
    out["Sdd"] = [math.fsum(a * a) for a in d]                   # the square of a float32 is exact in binary64
    out["abs_dd"] = list(out["Sdd"])
    return out


def remove_motion(u, v, w, centre, t, M):
    """(ru, rv, rw, stats): res_r = (float)((double)d_r - (t_r + ((M_r0 X + M_r1 Y) + M_r2 Z))), every operation rounded on its own"""
    d, h, w_ = u.shape
    Z, Y, X = np.meshgrid(np.arange(d, dtype=F64) - F64(centre[2]), np.arange(h, dtype=F64) - F64(centre[1]),
                          np.arange(w_, dtype=F64) - F64(centre[0]), indexing="ij")
    M = np.asarray(M, F64).reshape(3, 3)
    res = []
    for r, comp in enumerate((u, v, w)):
        fitted = F64(t[r]) + ((M[r, 0] * X + M[r, 1] * Y) + M[r, 2] * Z)
        res.append((comp.astype(F64) - fitted).astype(F32))
    ok = ~(np.isnan(res[0]) | np.isnan(res[1]) | np.isnan(res[2]))
    sq = np.concatenate([a[ok].astype(F64) ** 2 for a in res])
    stats = {"present": int(ok.sum()), "sum_sq": math.fsum(sq),
             "max_abs": float(max(np.abs(a[ok]).max() for a in res)) if ok.any() else float("nan")}
    return res[0], res[1], res[2], stats


def centred_coordinates(shape, mask):
    return np.stack([c[mask].astype(F64) * 0.5 for c in doubled_coordinates(shape)], axis=1)       # [n, 3]


def affine_lstsq(u, v, w, mask):
    """(t[3], M[3, 3], normal matrix) of d ~ t + M X over the masked voxels by numpy.linalg.lstsq"""
    X = centred_coordinates(u.shape, mask)
    A = np.concatenate([np.ones((len(X), 1)), X], axis=1)
    D = np.stack([a[mask].astype(F64) for a in (u, v, w)], axis=1)
    sol = np.linalg.lstsq(A, D, rcond=None)[0]                    # [4, 3]
    return sol[0], sol[1:].T.copy(), A.T @ A


def kabsch(u, v, w, mask):
    """(R, t, singular values) of the rotation that brings the centred X closest to the centred X + d, by numpy.linalg.svd"""
    X = centred_coordinates(u.shape, mask)
    D = np.stack([a[mask].astype(F64) for a in (u, v, w)], axis=1)
    xb, db = X.mean(axis=0), D.mean(axis=0)
    Xc, Yc = X - xb, (X + D) - (xb + db)
    B = Yc.T @ Xc                                                 # sum y x^T
    U, S, Vt = np.linalg.svd(B)
    fix = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ fix @ Vt
    return R, db - (R - np.eye(3)) @ xb, S


# ---- constructions the tests share -----------------------------------------------------------------------------------------------------

def affine_field(shape, M, t, dtype=np.float64):
    d, h, w = shape
    X2, Y2, Z2 = doubled_coordinates(shape)
    X, Y, Z = (c.astype(np.float64) * 0.5 for c in (X2, Y2, Z2))
    return [(t[r] + M[r, 0] * X + M[r, 1] * Y + M[r, 2] * Z).astype(dtype) for r in range(3)]


def holes(shape, seed, fraction=0.10):
    return np.random.default_rng(seed).random(shape) < fraction


def rotation(angle, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
