"""numpy restatement of f3d_validate_displacement (include/f3d.h), in float32, operation for operation: the 26-slot neighbour list
padded with +inf and sorted by np.sort, the even and odd median rule by index, + float32(0) on stored medians.  The device must equal it
bit for bit except for the sign of a zero that the definition leaves open nowhere in what is stored (r is built from absolute values,
a stored median has had +0 added, a kept voxel is a copy).

validate() is vectorised (prepare() holds what does not depend on threshold, min_neighbours and mode, classify() the rest);
validate_loop() builds every neighbour list explicitly in Python and is what tests/test_outlier_cpu.py holds
validate() against."""
import itertools

import numpy as np

F32 = np.float32
INF = F32(np.inf)
MARK, REPLACE = 1, 2
MODES = {"mark": MARK, "replace": REPLACE}
OFFSETS = [(i, j, k) for k in (-1, 0, 1) for j in (-1, 0, 1) for i in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]   # (dx, dy, dz)


def present_mask(u, v, w, weight=None, weight_min=0.8):
    m = ~(np.isnan(u) | np.isnan(v) | np.isnan(w))
    if weight is not None:
        with np.errstate(invalid="ignore"):
            m &= np.asarray(weight, F32) >= F32(weight_min)          # a NaN weight fails the comparison
    return m


def _shifted(a, present, step, off):
    """a at p + step * off where that point is inside the volume and present, +inf elsewhere"""
    d, h, w = a.shape
    out = np.full(a.shape, INF, F32)
    dx, dy, dz = (step * o for o in off)
    zs, ys, xs = (slice(max(0, -s), max(0, n - max(0, s))) for s, n in ((dz, d), (dy, h), (dx, w)))
    zt, yt, xt = (slice(sl.start + s, sl.stop + s) for sl, s in ((zs, dz), (ys, dy), (xs, dx)))
    if zs.stop <= zs.start or ys.stop <= ys.start or xs.stop <= xs.start:
        return out
    out[zs, ys, xs] = np.where(present[zt, yt, xt], a[zt, yt, xt], INF)
    return out


def _median_by_index(s, k):
    """the median of s[0 .. k) along axis 0 of the ascending s, per voxel; 0 where k == 0 (nothing reads it)"""
    kk = np.maximum(k, 1)
    lo = np.take_along_axis(s, ((kk - 1) // 2)[None], 0)[0]
    hi = np.take_along_axis(s, (kk // 2)[None], 0)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        even = F32(0.5) * (lo + hi)
    return np.where(k == 0, F32(0), np.where(kk % 2 == 1, hi, even)).astype(F32)


def neighbour_medians(a, present, step):
    """(med, rm, k) of one component"""
    lists = np.stack([_shifted(a, present, step, off) for off in OFFSETS])
    k = np.isfinite(lists).sum(0)
    s = np.sort(lists, axis=0)
    med = _median_by_index(s, k)
    with np.errstate(invalid="ignore"):
        res = np.sort(np.abs(lists - med[None]), axis=0)              # inf - med = inf: the pads stay last
    return med, _median_by_index(res, k), k


def prepare(u, v, w, weight=None, weight_min=0.8, step=1, eps=0.1):
    """everything that does not depend on threshold, min_neighbours and mode: (fields, present, k, r, medians)"""
    u, v, w = (np.ascontiguousarray(a, F32) for a in (u, v, w))
    present = present_mask(u, v, w, weight, weight_min)
    eps = F32(eps)
    rs, meds, k = [], [], None
    for a in (u, v, w):
        med, rm, k = neighbour_medians(a, present, step)
        with np.errstate(invalid="ignore", over="ignore"):
            rs.append(np.abs(a - med) / (rm + eps))
        meds.append(med)
    with np.errstate(invalid="ignore"):
        r = np.fmax(np.fmax(rs[0], rs[1]), rs[2]).astype(F32)
    return (u, v, w), present, k, r, meds


def classify(prepared, threshold=2.0, min_neighbours=9, mode=REPLACE):
    """returns (r, vu, vv, vw, stats): stats a dict present, tested, outliers, replaced, undefined, r_max (float32 or NaN)"""
    fields, present, k, r, meds = prepared
    enough = k >= min_neighbours
    tested = present & enough
    with np.errstate(invalid="ignore"):
        outlier = tested & (r > F32(threshold))
    kept = present & ~outlier
    median = ~kept & enough & (mode == REPLACE)
    nan = F32(np.nan)
    out = [np.where(kept, a, np.where(median, med + F32(0), nan)).astype(F32) for a, med in zip(fields, meds)]
    r_out = np.where(tested, r, nan).astype(F32)
    stats = dict(present=int(present.sum()), tested=int(tested.sum()), outliers=int(outlier.sum()), replaced=int(median.sum()),
                 undefined=int(np.isnan(out[0]).sum()), r_max=F32(r[tested].max()) if tested.any() else nan)
    return (r_out, *out, stats)


def validate(u, v, w, weight=None, weight_min=0.8, step=1, eps=0.1, threshold=2.0, min_neighbours=9, mode=REPLACE):
    return classify(prepare(u, v, w, weight, weight_min, step, eps), threshold, min_neighbours, mode)


def fill(u, v, w, passes, step=1, eps=0.1, min_neighbours=9):
    """the fill passes of the drivers: validate() with threshold inf, no weight, REPLACE, until nothing is undefined or the count stops
    falling; returns (u, v, w, replaced in all passes, undefined at the end, the undefined count after every pass run)"""
    undefined = int(np.isnan(u).sum())
    replaced, history = 0, []
    for _ in range(passes):
        if not undefined:
            break
        _, u, v, w, st = validate(u, v, w, None, 0.0, step, eps, np.inf, min_neighbours, REPLACE)
        replaced += st["replaced"]
        fell = st["undefined"] < undefined
        undefined = st["undefined"]
        history.append(undefined)
        if not fell:
            break
    return u, v, w, replaced, undefined, history


def validate_loop(u, v, w, weight=None, weight_min=0.8, step=1, eps=0.1, threshold=2.0, min_neighbours=9, mode=REPLACE):
    """the same, voxel by voxel, every neighbour list built explicitly"""
    u, v, w = (np.ascontiguousarray(a, F32) for a in (u, v, w))
    d, h, wd = u.shape
    present = present_mask(u, v, w, weight, weight_min)
    eps, threshold, nan = F32(eps), F32(threshold), F32(np.nan)
    r_out = np.full(u.shape, nan, F32)
    out = [np.full(u.shape, nan, F32) for _ in range(3)]
    st = dict(present=0, tested=0, outliers=0, replaced=0, undefined=0, r_max=nan)

    def median(vals):
        s = sorted(vals)
        n = len(s)
        return s[(n - 1) // 2] if n % 2 else F32(0.5) * F32(s[n // 2 - 1] + s[n // 2])

    with np.errstate(all="ignore"):
        for z, y, x in itertools.product(range(d), range(h), range(wd)):
            nb = [(z + step * k, y + step * j, x + step * i) for i, j, k in OFFSETS]
            nb = [q for q in nb if 0 <= q[0] < d and 0 <= q[1] < h and 0 <= q[2] < wd and present[q]]
            k = len(nb)
            meds, r = [], F32(-np.inf)
            for a in (u, v, w):
                if k:
                    med = median([a[q] for q in nb])
                    rm = median([F32(abs(F32(a[q] - med))) for q in nb])
                    r = np.fmax(r, F32(abs(F32(a[z, y, x] - med))) / F32(rm + eps))
                    meds.append(med)
            p = bool(present[z, y, x])
            tested = p and k >= min_neighbours
            outlier = tested and bool(r > threshold)
            kept = p and not outlier
            gets = (not kept) and mode == REPLACE and k >= min_neighbours
            st["present"] += p
            st["tested"] += tested
            st["outliers"] += outlier
            st["replaced"] += gets
            if tested:
                r_out[z, y, x] = r
                st["r_max"] = r if np.isnan(st["r_max"]) else max(st["r_max"], r)
            for c, a in enumerate((u, v, w)):
                if kept:
                    out[c][z, y, x] = a[z, y, x]
                elif gets:
                    out[c][z, y, x] = F32(meds[c] + F32(0))
            st["undefined"] += bool(np.isnan(out[0][z, y, x]))
    return (r_out, *out, st)
