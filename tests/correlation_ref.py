"""Numpy restatement of include/f3d.h's f3d_local_correlation, the checker of the kernel.  It imports nothing from the product.

Per voxel of two [z, y, x] float32 volumes a and b: present = neither is NaN; m = 1, A = float64(a), B = float64(b) where present, all
+0 elsewhere; the seven quantities m, A, B, A*A, B*B, A*B, (A - B)*(A - B) in float64; their sums over the (2r+1)^3 window formed
separably (x, then y, then z) as sums of shifted slices of a zero-padded array, in ascending order of the coordinate, every addition
rounded on its own; then the float32 tail.  So this agrees with the kernel bit for bit (NaN positions, not payloads)."""
import numpy as np

F32 = np.float32
ZNCC, RMSD = 1, 2
FLAT_FLOOR = 2.0 ** -40


def same_bits(a, b):
    """equal as float32 values with NaN at the same positions (payloads not compared); -0 and +0 differ"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def axis_sum(q, r, axis):
    """(((t_-r + t_-r+1) + ...) + t_r) along `axis` of a float64 array, terms outside it +0"""
    n = q.shape[axis]
    pad = [(0, 0)] * q.ndim
    pad[axis] = (r, r)
    p = np.pad(q, pad)  # +0
    take = lambda i: np.take(p, np.arange(i, i + n), axis=axis)
    acc = take(0) + take(1)
    for i in range(2, 2 * r + 1):
        acc = acc + take(i)
    return acc


def window_sum(q, r):
    return axis_sum(axis_sum(axis_sum(q, r, 2), r, 1), r, 0)


def window_sums(a, b, r):
    """present, and n, Sa, Sb, Saa, Sbb, Sab, Sdd (float64 [z, y, x])"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    present = ~(np.isnan(a) | np.isnan(b))
    with np.errstate(invalid="ignore", over="ignore"):
        A = np.where(present, a.astype(np.float64), 0.0)
        B = np.where(present, b.astype(np.float64), 0.0)
        d = A - B
        qs = (present.astype(np.float64), A, B, A * A, B * B, A * B, d * d)
        return present, [window_sum(q, r) for q in qs]


def local_correlation(a, b, radius, threshold=0.8):
    """(zncc, rmsd, stats) of two [z, y, x] volumes: float32 arrays, NaN where the centre is absent (and zncc where the window is
    flat), and a dict with the statistics of f3d_correlation_stats"""
    present, (n, Sa, Sb, Saa, Sbb, Sab, Sdd) = window_sums(a, b, radius)
    nan = F32(np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        rmsd = np.sqrt(Sdd.astype(F32) / n.astype(F32)).astype(F32)
        nSaa, nSbb = n * Saa, n * Sbb
        va = nSaa - Sa * Sa
        vb = nSbb - Sb * Sb
        c = n * Sab - Sa * Sb
        flat = ~(va > FLAT_FLOOR * nSaa) | ~(vb > FLAT_FLOOR * nSbb)
        zncc = (c.astype(F32) / (np.sqrt(va.astype(F32)) * np.sqrt(vb.astype(F32)))).astype(F32)
    zncc = np.where(present & ~flat, zncc, nan).astype(F32)
    rmsd = np.where(present, rmsd, nan).astype(F32)
    defined = ~np.isnan(zncc)
    with np.errstate(invalid="ignore"):
        stats = {
            "defined": int(defined.sum()),
            "lost": int((~present).sum()),
            "below": int((defined & (zncc < F32(threshold))).sum()),
            "zncc_min": float(zncc[defined].min()) if defined.any() else float("nan"),
            "rmsd_max": float(rmsd[present].max()) if present.any() else float("nan"),
            "zncc_sum": float(zncc[defined].astype(np.float64).sum()),
            "zncc_abs_sum": float(np.abs(zncc[defined].astype(np.float64)).sum()),  # the scale of zncc_sum's rounding
        }
    return zncc, rmsd, stats
