"""numpy restatement of the per-label motion of include/f3d.h and include/f3d_host.h, written from the headers: the classes of
f3d_label_info, the quantisation q = rint(d * 2^14) in float32, the sums as Python integers (object arrays, so nothing can overflow
or round), float(int) for the single rounding to binary64, the recentring of f3d_motion_solve_labels, and the subtraction of
f3d_remove_label_motion in motion_ref.py's order with a per-label centre.  At the end, the label volumes the tests share."""
import math

import numpy as np

from motion_ref import SXX_ORDER, doubled_coordinates

F32 = np.float32
F64 = np.float64
OK, EMPTY, SMALL, DEGENERATE = 0, 1, 2, 3
INFO = ("background", "foreign", "absent", "out_of_range", "used")


def classify(u, v, w, labels, n_labels, weight=None, weight_min=0.8):
    """(the mask of the voxels that take part, the dict of f3d_label_info); the classes are exclusive and taken in the header's order"""
    labels = np.asarray(labels).astype(np.int64)
    background = labels == 0
    foreign = (labels < 0) | (labels > n_labels)
    ranged = ~background & ~foreign
    here = ~(np.isnan(u) | np.isnan(v) | np.isnan(w))
    if weight is not None:
        with np.errstate(invalid="ignore"):
            here &= weight >= F32(weight_min)                   # a NaN weight fails the comparison
    absent = ranged & ~here
    with np.errstate(invalid="ignore"):
        small = (np.abs(u) < F32(1024)) & (np.abs(v) < F32(1024)) & (np.abs(w) < F32(1024))
    out_of_range = ranged & here & ~small
    used = ranged & here & small
    info = {k: int(m.sum()) for k, m in zip(INFO, (background, foreign, absent, out_of_range, used))}
    assert sum(info.values()) == labels.size
    return used, info


def quantise(a):
    """q = (int)rintf(a * 16384.0f): the float32 product (exact), numpy's rint (to nearest, ties to even)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(a.astype(F32) * F32(16384.0))


def label_integers(u, v, w, labels, n_labels, weight=None, weight_min=0.8):
    """(per label the dict of exact Python integers n, x2[3], xx4[6], Id[3], Ixd[9], Idd[3], info)"""
    used, info = classify(u, v, w, labels, n_labels, weight, weight_min)
    lab = np.asarray(labels).astype(np.int64)[used]
    c2 = [c[used].astype(object) for c in doubled_coordinates(u.shape)]
    q = [np.array([int(x) for x in quantise(a[used])], dtype=object) for a in (u, v, w)]
    assert all(abs(x) <= 2 ** 24 for a in q for x in a)
    out = []
    order = np.argsort(lab, kind="stable")
    lab_sorted = lab[order]
    starts = np.searchsorted(lab_sorted, np.arange(1, n_labels + 2))
    for L in range(n_labels):
        idx = order[starts[L]:starts[L + 1]]
        c = [a[idx] for a in c2]
        d = [a[idx] for a in q]
        isum = lambda a: int(a.sum()) if len(a) else 0
        out.append({"n": len(idx), "x2": [isum(a) for a in c], "xx4": [isum(c[i] * c[k]) for i, k in SXX_ORDER],
                    "Id": [isum(a) for a in d], "Ixd": [isum(c[i] * d[j]) for i in range(3) for j in range(3)],
                    "Idd": [isum(a * a) for a in d]})
    return out, info


def scaled(i, exponent):
    """the integer rounded to binary64 once (float(int) rounds to nearest even), then scaled by a power of two"""
    return math.ldexp(float(i), exponent)


def label_sums(u, v, w, labels, n_labels, weight=None, weight_min=0.8):
    """(per label the dict n, Sx, Sxx, Sd, Sxd, Sdd of struct f3d_motion_sums, info)"""
    ints, info = label_integers(u, v, w, labels, n_labels, weight, weight_min)
    out = [{"n": s["n"], "Sx": [scaled(i, -1) for i in s["x2"]], "Sxx": [scaled(i, -2) for i in s["xx4"]],
            "Sd": [scaled(i, -14) for i in s["Id"]], "Sxd": [scaled(i, -15) for i in s["Ixd"]],
            "Sdd": [scaled(i, -28) for i in s["Idd"]]} for s in ints]
    return out, info


def recentre(sums, volume_centre, t, M):
    """(centre, t) of an OK label of f3d_motion_solve_labels from the fit (t, M) about the volume centre, in the header's order"""
    n = F64(sums["n"])
    xb = [F64(s) / n for s in sums["Sx"]]
    M = np.asarray(M, F64).reshape(3, 3)
    centre = [F64(volume_centre[a]) + xb[a] for a in range(3)]
    t = [F64(t[r]) + ((M[r, 0] * xb[0] + M[r, 1] * xb[1]) + M[r, 2] * xb[2]) for r in range(3)]
    return [float(c) for c in centre], [float(x) for x in t]


def remove_label_motion(u, v, w, labels, centre, t, M, ok):
    """(ru, rv, rw, stats) with centre [N, 3], t [N, 3], M [N, 3, 3], ok [N] per label:
    res_r = (float)((double)d_r - (t_r + ((M_r0 X + M_r1 Y) + M_r2 Z))) with X = x - centre_L[0], every operation rounded on its own; NaN
    where the label is not in 1 .. N or not ok"""
    n = len(ok)
    d, h, w_ = u.shape
    lab = np.asarray(labels).astype(np.int64)
    valid = (lab >= 1) & (lab <= n)
    row = np.where(valid, lab - 1, 0)
    valid &= np.asarray(ok, bool)[row]
    centre, t, M = np.asarray(centre, F64).reshape(n, 3), np.asarray(t, F64).reshape(n, 3), np.asarray(M, F64).reshape(n, 3, 3)
    z, y, x = np.meshgrid(np.arange(d, dtype=F64), np.arange(h, dtype=F64), np.arange(w_, dtype=F64), indexing="ij")
    X, Y, Z = x - centre[row, 0], y - centre[row, 1], z - centre[row, 2]
    res = []
    for r, comp in enumerate((u, v, w)):
        fitted = t[row, r] + ((M[row, r, 0] * X + M[row, r, 1] * Y) + M[row, r, 2] * Z)
        out = (comp.astype(F64) - fitted).astype(F32)
        out[~valid] = np.nan
        res.append(out)
    good = ~(np.isnan(res[0]) | np.isnan(res[1]) | np.isnan(res[2]))
    sq = np.concatenate([a[good].astype(F64) ** 2 for a in res])
    stats = {"present": int(good.sum()), "sum_sq": math.fsum(sq),
             "max_abs": float(max(np.abs(a[good]).max() for a in res)) if good.any() else float("nan")}
    return res[0], res[1], res[2], stats


# ---- label volumes the tests share -------------------------------------------------------------------------------------------------------

def voronoi(shape, seeds, seed=0):
    """labels 1 .. seeds [z, y, x] int32: the cell of the nearest of `seeds` random points"""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    pts = rng.random((seeds, 3)) * np.array([d, h, w])
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    best = np.full(shape, np.inf)
    lab = np.zeros(shape, np.int32)
    for k, p in enumerate(pts):
        dist = (z - p[0]) ** 2 + (y - p[1]) ** 2 + (x - p[2]) ** 2
        closer = dist < best
        best[closer] = dist[closer]
        lab[closer] = k + 1
    return lab
