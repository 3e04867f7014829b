"""Subset correlation (include/f3d_subset_match.h and f3d_subset_match_table of include/f3d_host.h) stated twice.

subset_match() is the numpy restatement of the header's rule in the header's operation order: binary64 with every operation rounded
on its own, and every sum over the window taken by the 256-lane partition and the tree the header fixes, so the device is held to it
bit for bit.  table() restates the host table the same way.

plain() is an independent statement of the same method for small windows: Python loops over the voxels, the Keys kernel written as
a function of the distance, the normal equations through numpy.linalg and the composition through 4 x 4 homogeneous matrices.  It
shares no helper with the restatement and keeps no summation order, so the two agree within rounding, not bit for bit."""
import math

import numpy as np

LANES = 256
TRANSLATION, AFFINE = 0, 1
OK, NAN, FLAT, FLAT_TARGET, SINGULAR, OUTSIDE, LOST, NOT_CONVERGED, NO_START, LOW = range(10)
STATUS = ("ok", "nan", "flat", "flat_target", "singular", "outside", "lost", "not_converged", "no_start", "low")
RECORD = np.dtype([("p", np.float64, 12), ("zncc", np.float64), ("step", np.float64), ("df", np.float64), ("dg", np.float64),
                   ("status", np.int32), ("iterations", np.int32), ("nan", np.int32), ("reserved", np.int32)])
ROW = np.dtype([("position", np.int32, 3), ("status", np.int32), ("iterations", np.int32), ("reserved", np.int32), ("zncc", np.float64),
                ("u", np.float32), ("v", np.float32), ("w", np.float32), ("grad", np.float32, 9), ("diff", np.float32, 3),
                ("reserved2", np.int32)])
assert RECORD.itemsize == 144 and ROW.itemsize == 96


class Grid:
    def __init__(self, origin, step, counts, window):
        self.origin, self.step, self.counts, self.window = tuple(int(o) for o in origin), int(step), tuple(int(c) for c in counts), int(window)

    @property
    def nodes(self):
        return self.counts[0] * self.counts[1] * self.counts[2]

    def positions(self):
        """(x, y, z) of every node, x fastest"""
        (ox, oy, oz), s, (nx, ny, nz) = self.origin, self.step, self.counts
        return [(ox + i * s, oy + j * s, oz + k * s) for k in range(nz) for j in range(ny) for i in range(nx)]


def default_grid(dims, step, window):
    """the grid subset_grid of the package and f3d_subset_match_layout lay: as many nodes as fit with window + 1 to each face, centred"""
    first, count = [], []
    for n in dims:
        reach = window + 1
        room = n - 1 - 2 * reach
        assert room >= 0
        o = reach + (room % step) // 2
        first.append(o)
        count.append((n - 1 - reach - o) // step + 1)
    return Grid(first, step, count, window)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def lane_sum(terms):
    """The header's sum of terms[i] over the window voxels i (axis 0; any further axes are summed alike, entry by entry)"""
    terms = np.asarray(terms, np.float64)
    n = terms.shape[0]
    rounds = (n + LANES - 1) // LANES
    padded = np.zeros((rounds * LANES,) + terms.shape[1:], np.float64)      # + 0 behind a lane's last voxel changes nothing
    padded[:n] = terms
    padded = padded.reshape((rounds, LANES) + terms.shape[1:])
    acc = np.zeros((LANES,) + terms.shape[1:], np.float64)
    for r in range(rounds):
        acc = acc + padded[r]
    half = LANES // 2
    while half:
        acc[:half] = acc[:half] + acc[half:2 * half]
        half //= 2
    return acc[0]


def offsets(W):
    """xi of every window voxel, x fastest: three int arrays"""
    r = np.arange(-W, W + 1)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def weights(t):
    return ((((2.0 - t) * t - 1.0) * t) * 0.5, (((3.0 * t - 5.0) * t) * t + 2.0) * 0.5, (((4.0 - 3.0 * t) * t + 1.0) * t) * 0.5,
            (((t - 1.0) * t) * t) * 0.5)


def line(w, q):
    return ((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2]) + w[3] * q[3]


def factor(H):
    """Cholesky in the header's order -> L, or None when a pivot is not positive"""
    m = H.shape[0]
    L = np.zeros((m, m), np.float64)
    for j in range(m):
        for k in range(j):
            v = H[j, k]
            for q in range(k):
                v = v - L[j, q] * L[k, q]
            L[j, k] = v / L[k, k]
        d = H[j, j]
        for q in range(j):
            d = d - L[j, q] * L[j, q]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
    return L


def solve(L, rhs):
    m = L.shape[0]
    y = np.zeros(m, np.float64)
    for j in range(m):
        v = rhs[j]
        for q in range(j):
            v = v - L[j, q] * y[q]
        y[j] = v / L[j, j]
    for j in range(m - 1, -1, -1):
        v = y[j]
        for q in range(j + 1, m):
            v = v - L[q, j] * y[q]
        y[j] = v / L[j, j]
    dp = np.zeros(12, np.float64)
    if m == 3:
        dp[0::4] = -y
    else:
        dp[:] = -y
    return dp


def compose(p, dp):
    """p o dp^-1 -> the new p, or None when the determinant is 0"""
    eye = np.eye(3)
    A = eye + p.reshape(3, 4)[:, 1:]
    B = eye + dp.reshape(3, 4)[:, 1:]
    C = np.zeros((3, 3), np.float64)
    C[0, 0] = B[1, 1] * B[2, 2] - B[1, 2] * B[2, 1]
    C[0, 1] = B[0, 2] * B[2, 1] - B[0, 1] * B[2, 2]
    C[0, 2] = B[0, 1] * B[1, 2] - B[0, 2] * B[1, 1]
    C[1, 0] = B[1, 2] * B[2, 0] - B[1, 0] * B[2, 2]
    C[1, 1] = B[0, 0] * B[2, 2] - B[0, 2] * B[2, 0]
    C[1, 2] = B[0, 2] * B[1, 0] - B[0, 0] * B[1, 2]
    C[2, 0] = B[1, 0] * B[2, 1] - B[1, 1] * B[2, 0]
    C[2, 1] = B[0, 1] * B[2, 0] - B[0, 0] * B[2, 1]
    C[2, 2] = B[0, 0] * B[1, 1] - B[0, 1] * B[1, 0]
    det = (B[0, 0] * C[0, 0] + B[0, 1] * C[1, 0]) + B[0, 2] * C[2, 0]
    if det == 0.0:
        return None
    V = C / det
    N = np.zeros((3, 3), np.float64)
    for r in range(3):
        for c in range(3):
            N[r, c] = (A[r, 0] * V[0, c] + A[r, 1] * V[1, c]) + A[r, 2] * V[2, c]
    out = np.zeros(12, np.float64)
    for r in range(3):
        out[4 * r] = p[4 * r] - ((N[r, 0] * dp[0] + N[r, 1] * dp[4]) + N[r, 2] * dp[8])
        for c in range(3):
            out[4 * r + 1 + c] = N[r, c] - eye[r, c]
    return out


def node_match(a, b, c, W, model, start, max_iterations, tolerance, reach):
    """one node -> a RECORD scalar (as a 0-d structured array)"""
    rec = np.zeros((), RECORD)
    p = np.zeros(12, np.float64) if start is None else np.array(start, np.float64)
    rec["p"] = p
    if np.isnan(p).any():
        rec["status"] = NO_START
        return rec
    D, H_, Wd = a.shape
    cx, cy, cz = c
    xi = offsets(W)
    n = xi[0].size
    X, Y, Z = cx + xi[0], cy + xi[1], cz + xi[2]
    a64 = a.astype(np.float64)
    f = a64[Z, Y, X]
    nans = int(np.isnan(f).sum())
    rec["nan"] = nans
    fsum = lane_sum(f)
    if nans:
        rec["status"] = NAN
        return rec
    fm = fsum / np.float64(n)
    F = f - fm
    df = np.sqrt(lane_sum(F * F))
    rec["df"] = df
    if df == 0.0:
        rec["status"] = FLAT
        return rec
    fx = (a64[Z, Y, X + 1] - a64[Z, Y, X - 1]) * 0.5
    fy = (a64[Z, Y + 1, X] - a64[Z, Y - 1, X]) * 0.5
    fz = (a64[Z + 1, Y, X] - a64[Z - 1, Y, X]) * 0.5
    e = [x.astype(np.float64) for x in xi]
    if model == TRANSLATION:
        J = np.stack([fx, fy, fz], axis=1)
    else:
        J = np.stack([col for d in (fx, fy, fz) for col in (d, d * e[0], d * e[1], d * e[2])], axis=1)
    m = J.shape[1]
    Hm = lane_sum(J[:, :, None] * J[:, None, :])
    L = factor(Hm)
    if L is None:
        rec["status"] = SINGULAR
        return rec
    p0 = p.copy()
    b64 = b.astype(np.float64)
    iteration = 0
    while True:
        iteration += 1
        rec["iterations"] = iteration
        pts = [(c[k] + xi[k]).astype(np.float64) + (((p[4 * k] + p[4 * k + 1] * e[0]) + p[4 * k + 2] * e[1]) + p[4 * k + 3] * e[2])
               for k in range(3)]
        base = [np.floor(q) for q in pts]
        inside = np.ones(n, bool)
        for q, size in zip(base, (Wd, H_, D)):
            inside &= (q >= 1.0) & (q <= float(size - 3))          # a NaN fails
        if not inside.all():
            rec["status"] = OUTSIDE
            return rec
        w = [weights(q - q0) for q, q0 in zip(pts, base)]
        ix, iy, iz = (q.astype(np.int64) - 1 for q in base)
        planes = []
        for kz in range(4):
            rows = [line(w[0], [b64[iz + kz, iy + ky, ix + kx] for kx in range(4)]) for ky in range(4)]
            planes.append(line(w[1], rows))
        g = line(w[2], planes)
        gsum = lane_sum(g)
        if np.isnan(gsum):
            rec["status"] = NAN
            return rec
        gm = gsum / np.float64(n)
        G = g - gm
        sums = lane_sum(np.stack([G * G, F * G], axis=1))
        dg = np.sqrt(sums[0])
        rec["dg"] = dg
        if dg == 0.0:
            rec["status"] = FLAT_TARGET
            return rec
        rec["zncc"] = sums[1] / (df * dg)
        ratio = df / dg
        res = F - ratio * G
        rhs = lane_sum(J * res[:, None])
        dp = solve(L, rhs)
        new = compose(p, dp)
        if new is None:
            rec["status"] = SINGULAR
            return rec
        p = new
        rec["p"] = p
        grads = np.float64(0.0)
        for k in range(12):
            if k % 4:
                grads = grads + dp[k] * dp[k]
        step = np.sqrt(((dp[0] * dp[0] + dp[4] * dp[4]) + dp[8] * dp[8]) + (np.float64(W) * np.float64(W)) * grads)
        rec["step"] = step
        du, dv, dw = p[0] - p0[0], p[4] - p0[4], p[8] - p0[8]
        if step < tolerance:
            rec["status"] = OK
            return rec
        if np.sqrt((du * du + dv * dv) + dw * dw) > reach:
            rec["status"] = LOST
            return rec
        if iteration == max_iterations:
            rec["status"] = NOT_CONVERGED
            return rec


def subset_match(a, b, grid, model=AFFINE, start=None, max_iterations=20, tolerance=1e-3, reach=None):
    """-> (records as RECORD [nodes], info dict) of volumes a, b [z, y, x] float32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    reach = float(grid.window) if reach is None else float(reach)
    records = np.zeros(grid.nodes, RECORD)
    if start is not None:
        start = np.asarray(start, np.float64).reshape(grid.nodes, 12)
    with np.errstate(all="ignore"):
        for node, c in enumerate(grid.positions()):
            records[node] = node_match(a, b, c, grid.window, model, None if start is None else start[node], int(max_iterations),
                                       np.float64(tolerance), np.float64(reach))
    return records, info_of(records)


def info_of(records):
    return dict(nodes=len(records), status=[int((records["status"] == s).sum()) for s in range(9)],
                iterations=int(records["iterations"].astype(np.int64).sum()), nan=int(records["nan"].astype(np.int64).sum()))


# ---- the host table ----------------------------------------------------------------------------------------------------------------
def table(records, grid, min_zncc, compare=None):
    """f3d_subset_match_table: -> (rows as ROW [nodes], summary dict).  compare: three float32 node arrays or None."""
    rows = np.zeros(grid.nodes, ROW)
    counts = [0] * 10
    lengths, znccs = [], []
    nan32 = np.float32(np.nan)
    for i, (rec, pos) in enumerate(zip(records, grid.positions())):
        row = rows[i]
        row["position"] = pos
        status = int(rec["status"])
        if status == OK:
            if not np.isnan(rec["zncc"]):
                znccs.append(float(rec["zncc"]))
            if not rec["zncc"] >= min_zncc:
                status = LOW
        row["status"], row["iterations"], row["zncc"] = status, rec["iterations"], rec["zncc"]
        counts[status] += 1
        good = status == OK
        p = rec["p"]
        uvw = [np.float32(p[4 * k]) if good else nan32 for k in range(3)]
        row["u"], row["v"], row["w"] = uvw
        row["grad"] = [np.float32(p[4 * r + 1 + c]) if good else nan32 for r in range(3) for c in range(3)]
        if compare is None:
            row["diff"] = nan32
        else:
            d = [np.float64(np.asarray(compare[k], np.float32).ravel()[i]) - np.float64(uvw[k]) for k in range(3)]
            row["diff"] = [np.float32(x) for x in d]
            if good and not any(np.isnan(x) for x in d):
                lengths.append(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    summary = dict(nodes=grid.nodes, status=counts, compared=len(lengths), median_zncc=lower_median(znccs))
    total = np.float64(0.0)
    for x in lengths:
        total = total + x * x
    summary["rms"] = float(np.sqrt(total / np.float64(len(lengths)))) if lengths else float("nan")
    summary["median"] = lower_median(lengths)
    summary["p95"] = float(sorted(lengths)[(95 * len(lengths) + 99) // 100 - 1]) if lengths else float("nan")
    return rows, summary


def lower_median(values):
    return float(sorted(values)[(len(values) - 1) // 2]) if values else float("nan")


# ---- the independent statement --------------------------------------------------------------------------------------------------------
def plain(a, b, c, W, model, start=None, max_iterations=20, tolerance=1e-3, reach=None):
    """One node by textbook IC-GN in Python loops -> dict(p, zncc, step, status, iterations).  For small windows."""
    def keys(s):
        s = abs(s)
        if s < 1.0:
            return 1.5 * s ** 3 - 2.5 * s ** 2 + 1.0
        if s < 2.0:
            return -0.5 * s ** 3 + 2.5 * s ** 2 - 4.0 * s + 2.0
        return 0.0

    D, H_, Wd = a.shape
    reach = float(W) if reach is None else reach
    p = [0.0] * 12 if start is None else [float(x) for x in start]
    if any(math.isnan(x) for x in p):
        return dict(p=p, status=NO_START, iterations=0, zncc=0.0, step=0.0)
    vox = [(x, y, z) for z in range(-W, W + 1) for y in range(-W, W + 1) for x in range(-W, W + 1)]
    n = len(vox)
    f = [float(a[c[2] + z, c[1] + y, c[0] + x]) for x, y, z in vox]
    out = dict(p=p, iterations=0, zncc=0.0, step=0.0)
    if any(math.isnan(x) for x in f):
        return dict(out, status=NAN)
    fm = math.fsum(f) / n
    F = [x - fm for x in f]
    df = math.sqrt(math.fsum(x * x for x in F))
    if df == 0.0:
        return dict(out, status=FLAT)
    m = 3 if model == TRANSLATION else 12
    J = np.zeros((n, m))
    for i, (x, y, z) in enumerate(vox):
        X, Y, Z = c[0] + x, c[1] + y, c[2] + z
        grad = ((float(a[Z, Y, X + 1]) - float(a[Z, Y, X - 1])) / 2, (float(a[Z, Y + 1, X]) - float(a[Z, Y - 1, X])) / 2,
                (float(a[Z + 1, Y, X]) - float(a[Z - 1, Y, X])) / 2)
        J[i] = grad if m == 3 else [d * s for d in grad for s in (1, x, y, z)]
    Hm = J.T @ J
    try:
        np.linalg.cholesky(Hm)
    except np.linalg.LinAlgError:
        return dict(out, status=SINGULAR)

    def matrix(q):
        M = np.eye(4)
        for r in range(3):
            M[r, 3] = q[4 * r]
            for k in range(3):
                M[r, k] += q[4 * r + 1 + k]
        return M

    M, M0 = matrix(p), matrix(p)
    for iteration in range(1, max_iterations + 1):
        out["iterations"] = iteration
        g = []
        for x, y, z in vox:
            pt = M @ np.array([x, y, z, 1.0]) + np.array([c[0], c[1], c[2], 0.0])
            if not all(math.isfinite(q) for q in pt[:3]):
                return dict(out, status=OUTSIDE)
            lo = [math.floor(q) for q in pt[:3]]
            if not all(1 <= q <= size - 3 for q, size in zip(lo, (Wd, H_, D))):
                return dict(out, status=OUTSIDE)
            value = 0.0
            for kz in range(-1, 3):
                for ky in range(-1, 3):
                    for kx in range(-1, 3):
                        value += (keys(pt[0] - (lo[0] + kx)) * keys(pt[1] - (lo[1] + ky)) * keys(pt[2] - (lo[2] + kz))
                                  * float(b[lo[2] + kz, lo[1] + ky, lo[0] + kx]))
            g.append(value)
        if any(math.isnan(x) for x in g):
            return dict(out, status=NAN)
        gm = math.fsum(g) / n
        G = [x - gm for x in g]
        dg = math.sqrt(math.fsum(x * x for x in G))
        if dg == 0.0:
            return dict(out, status=FLAT_TARGET)
        out["zncc"] = math.fsum(x * y for x, y in zip(F, G)) / (df * dg)
        res = np.array([x - df / dg * y for x, y in zip(F, G)])
        dq = -np.linalg.solve(Hm, J.T @ res)
        full = [0.0] * 12
        if m == 3:
            full[0], full[4], full[8] = dq
        else:
            full = list(dq)
        Md = matrix(full)
        if np.linalg.det(Md[:3, :3]) == 0.0:
            return dict(out, status=SINGULAR)
        M = M @ np.linalg.inv(Md)
        p = [M[r, 3] if k == 0 else M[r, k - 1] - (1.0 if r == k - 1 else 0.0) for r in range(3) for k in range(4)]
        out["p"] = p
        out["step"] = math.sqrt(full[0] ** 2 + full[4] ** 2 + full[8] ** 2 + W * W * sum(full[k] ** 2 for k in range(12) if k % 4))
        if out["step"] < tolerance:
            return dict(out, status=OK)
        if np.linalg.norm(M[:3, 3] - M0[:3, 3]) > reach:
            return dict(out, status=LOST)
    return dict(out, status=NOT_CONVERGED)
