"""Plain numpy restatements of the block matching stage (include/f3d_block_match.h and f3d_block_match_solve of
include/f3d_host.h): the codes, the search of every node as a loop over nodes and shifts, the solve from records to rows, and the
expansion of node vectors.  Everything is integers, or floats with every operation rounded on its own, so the device and the host
library are held to these bit for bit.  brute_force() is a second, independent statement of the search for a tiny case."""
import numpy as np

RECORD_WORDS = 32
OK, FLAT, NONE = 0, 1, 2                                     # f3d_block_match_record.status
NODE_OK, NODE_FLAT, NODE_NONE, NODE_LOW, NODE_EDGE = 0, 1, 2, 3, 4   # f3d_block_match_node.status
NODE_DTYPE = np.dtype([("position", np.int32, 3), ("shift", np.int32, 3), ("status", np.int32), ("evaluated", np.int32),
                       ("outside", np.int32), ("flat", np.int32), ("zncc", np.float64), ("offset", np.float64, 3), ("u", np.float32),
                       ("v", np.float32), ("w", np.float32), ("reserved", np.int32)])
assert NODE_DTYPE.itemsize == 88


class Grid:
    def __init__(self, origin, step, counts, window, radii):
        self.origin, self.step, self.counts, self.window = tuple(origin), int(step), tuple(counts), int(window)
        self.radii = (radii,) * 3 if np.isscalar(radii) else tuple(radii)

    @property
    def nodes(self):
        return self.counts[0] * self.counts[1] * self.counts[2]

    def positions(self):
        """(x, y, z) of every node, x fastest"""
        (ox, oy, oz), s, (nx, ny, nz) = self.origin, self.step, self.counts
        return [(ox + i * s, oy + j * s, oz + k * s) for k in range(nz) for j in range(ny) for i in range(nx)]


def codes_of(volume, lo, hi, bins):
    """(codes as int64, NaN mask) of a float32 volume under the rule of f3d_histogram, with below -> 0, above -> bins - 1, NaN -> 0"""
    s = np.asarray(volume, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(bins) / (hi - lo)
    assert scale.dtype == np.float32
    nan = np.isnan(s)
    safe = np.where(nan, lo, s)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = (safe - lo) * scale
    inside = (safe >= lo) & (safe <= hi)
    binned = np.minimum(np.where(inside, scaled, np.float32(0)).astype(np.int64), bins - 1)
    codes = np.where(safe > hi, bins - 1, np.where(safe < lo, 0, binned))
    return np.where(nan, 0, codes).astype(np.int64), nan


def score_of(num, db):
    num = np.float64(num)
    squared = num * np.abs(num)
    return squared / np.float64(db)


def block_match(a, b, lo, hi, bins, grid, centre=None):
    """-> (records [nodes, 32] int32, info dict) of volumes a, b [z, y, x]"""
    ca, nan_a = codes_of(a, lo, hi, bins)
    cb, _ = codes_of(b, lo, hi, bins)
    D, H, Wd = ca.shape
    W, (rx, ry, rz) = grid.window, grid.radii
    side = 2 * W + 1
    n = side ** 3
    records = np.zeros((grid.nodes, RECORD_WORDS), np.int32)
    for node, (px, py, pz) in enumerate(grid.positions()):
        cx, cy, cz = (0, 0, 0) if centre is None else (int(c) for c in centre[node])
        rec = records[node]
        win = ca[pz - W:pz + W + 1, py - W:py + W + 1, px - W:px + W + 1]
        assert win.shape == (side,) * 3
        sa, saa = int(win.sum()), int((win * win).sum())
        rec[7], rec[8] = sa, saa
        rec[31] = int(nan_a[pz - W:pz + W + 1, py - W:py + W + 1, px - W:px + W + 1].sum())
        if n * saa - sa * sa == 0:
            rec[3] = FLAT
            continue

        def sums(dx, dy, dz):
            """None outside the box, else (sb, sbb, sab)"""
            x, y, z = px + cx + dx - W, py + cy + dy - W, pz + cz + dz - W
            if x < 0 or y < 0 or z < 0 or x + side > Wd or y + side > H or z + side > D:
                return None
            t = cb[z:z + side, y:y + side, x:x + side]
            return int(t.sum()), int((t * t).sum()), int((win * t).sum())

        best, best_score, best_sums = None, None, None
        evaluated = outside = flat = 0
        for dz in range(-rz, rz + 1):
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    s = sums(dx, dy, dz)
                    if s is None:
                        outside += 1
                        continue
                    db = n * s[1] - s[0] * s[0]
                    if db == 0:
                        flat += 1
                        continue
                    evaluated += 1
                    score = score_of(n * s[2] - sa * s[0], db)
                    if best is None or score > best_score:      # ties keep the earlier (smaller) index
                        best, best_score, best_sums = (dx, dy, dz), score, s
        rec[4], rec[5], rec[6] = evaluated, outside, flat
        if best is None:
            rec[3] = NONE
            continue
        rec[0:3] = cx + best[0], cy + best[1], cz + best[2]
        rec[9:12] = best_sums
        valid = 0
        for face, (axis, sign) in enumerate(((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))):
            d = list(best)
            d[axis] += sign
            if abs(d[axis]) > (rx, ry, rz)[axis]:
                continue
            s = sums(*d)
            if s is None or n * s[1] - s[0] * s[0] == 0:
                continue
            rec[12 + 3 * face:15 + 3 * face] = s
            valid |= 1 << face
        rec[30] = valid
    info = {"nodes": grid.nodes, "ok": int((records[:, 3] == OK).sum()), "flat_nodes": int((records[:, 3] == FLAT).sum()),
            "none_nodes": int((records[:, 3] == NONE).sum()), "evaluated": int(records[:, 4].sum(dtype=np.int64)),
            "outside": int(records[:, 5].sum(dtype=np.int64)), "flat": int(records[:, 6].sum(dtype=np.int64)),
            "nan": int(records[:, 31].sum(dtype=np.int64))}
    return records, info


def brute_force(a, b, lo, hi, bins, grid):
    """The best shift of every node of a tiny case, stated independently: codes by floor arithmetic on float64 (the rule's float32
    values are exact for the inputs of the test that uses this), the ZNCC itself in exact rationals, ordered as the rule orders it.
    -> [(shift or None, status)]"""
    from fractions import Fraction

    def code(s):
        if s != s or s < lo:
            return 0
        if s > hi:
            return bins - 1
        return min(int(np.floor((float(s) - lo) * bins / (hi - lo))), bins - 1)

    D, H, Wd = a.shape
    W, (rx, ry, rz) = grid.window, grid.radii
    out = []
    for (px, py, pz) in grid.positions():
        offsets = [(x, y, z) for z in range(-W, W + 1) for y in range(-W, W + 1) for x in range(-W, W + 1)]
        av = [code(a[pz + z, py + y, px + x]) for x, y, z in offsets]
        n = len(av)
        ma = Fraction(sum(av), n)
        va = sum((Fraction(c) - ma) ** 2 for c in av)
        if va == 0:
            out.append((None, FLAT))
            continue
        best = None
        for dz in range(-rz, rz + 1):
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    pts = [(px + dx + x, py + dy + y, pz + dz + z) for x, y, z in offsets]
                    if any(not (0 <= x < Wd and 0 <= y < H and 0 <= z < D) for x, y, z in pts):
                        continue
                    bv = [code(b[z, y, x]) for x, y, z in pts]
                    mb = Fraction(sum(bv), n)
                    vb = sum((Fraction(c) - mb) ** 2 for c in bv)
                    if vb == 0:
                        continue
                    cov = sum((Fraction(p) - ma) * (Fraction(q) - mb) for p, q in zip(av, bv))
                    signed_square = cov * abs(cov) / vb           # the order of cov / sqrt(va vb): va is common
                    if best is None or signed_square > best[0]:
                        best = (signed_square, (dx, dy, dz))
        out.append((best[1], OK) if best else (None, NONE))
    return out


def zncc_of(n, sa, da, sums):
    sb, sbb, sab = (int(s) for s in sums)
    num, db = n * sab - sa * sb, n * sbb - sb * sb
    product = np.float64(da) * np.float64(db)
    return np.float64(num) / np.sqrt(product)


def solve(records, grid, centre=None, min_zncc=0.5):
    """-> (rows as NODE_DTYPE, summary dict): f3d_block_match_solve restated"""
    n = (2 * grid.window + 1) ** 3
    rows = np.zeros(grid.nodes, NODE_DTYPE)
    for at, pos in enumerate(grid.positions()):
        r, row = records[at], rows[at]
        row["position"] = pos
        row["evaluated"], row["outside"], row["flat"] = r[4], r[5], r[6]
        row["zncc"] = np.nan
        row["u"] = row["v"] = row["w"] = np.nan
        if r[3] == FLAT:
            row["status"] = NODE_FLAT
            continue
        if r[3] != OK:
            row["status"] = NODE_NONE
            continue
        sa, saa = int(r[7]), int(r[8])
        da = n * saa - sa * sa
        z0 = zncc_of(n, sa, da, r[9:12])
        row["zncc"] = z0
        on_face = False
        for axis in range(3):
            row["shift"][axis] = r[axis]
            d = int(r[axis]) - (0 if centre is None else int(centre[at][axis]))
            if grid.radii[axis] > 0 and abs(d) == grid.radii[axis]:
                on_face = True
            offset = np.float64(0.0)
            if (int(r[30]) >> (2 * axis)) & 3 == 3:
                zm = zncc_of(n, sa, da, r[12 + 6 * axis:15 + 6 * axis])
                zp = zncc_of(n, sa, da, r[15 + 6 * axis:18 + 6 * axis])
                twice = np.float64(2.0) * z0
                curvature = (zm - twice) + zp
                if curvature < 0.0:
                    slope = zm - zp
                    offset = min(max(slope / (np.float64(2.0) * curvature), np.float64(-0.5)), np.float64(0.5))
            row["offset"][axis] = offset
        row["status"] = NODE_LOW if z0 < min_zncc else (NODE_EDGE if on_face else NODE_OK)
        if row["status"] != NODE_LOW:
            for name, axis in (("u", 0), ("v", 1), ("w", 2)):
                row[name] = np.float32(np.float64(row["shift"][axis]) + row["offset"][axis])
    status = rows["status"]
    summary = {"nodes": grid.nodes, "ok": int((status == NODE_OK).sum()), "flat": int((status == NODE_FLAT).sum()),
               "none": int((status == NODE_NONE).sum()), "low": int((status == NODE_LOW).sum()), "edge": int((status == NODE_EDGE).sum())}
    return rows, summary


def _axis(n_voxels, origin, step, count):
    t = (np.arange(n_voxels, dtype=np.float32) - np.float32(origin)) / np.float32(step)
    lower = np.clip(np.floor(t).astype(np.int64), 0, max(count - 2, 0))
    fraction = np.clip(t - lower.astype(np.float32), np.float32(0), np.float32(1))
    assert t.dtype == fraction.dtype == np.float32
    return lower, fraction


def _lerp(p, q, f):
    with np.errstate(invalid="ignore"):
        step = q - p
        part = f * step
        out = p + part
    assert out.dtype == np.float32
    return out


def expand_nodes(u, v, w, origin, step, dims):
    """node arrays [nz, ny, nx] float32 -> three dense [D, H, W] float32 volumes (f3d_expand_nodes restated)"""
    Wd, H, D = dims
    out = []
    for f in (u, v, w):
        f = np.asarray(f, np.float32)
        nz, ny, nx = f.shape
        i, fx = _axis(Wd, origin[0], step, nx)
        j, fy = _axis(H, origin[1], step, ny)
        k, fz = _axis(D, origin[2], step, nz)
        g = _lerp(f[:, :, i], f[:, :, i + 1], fx[None, None, :]) if nx > 1 else f[:, :, np.zeros(Wd, np.int64)]
        g = _lerp(g[:, j, :], g[:, j + 1, :], fy[None, :, None]) if ny > 1 else g[:, np.zeros(H, np.int64), :]
        g = _lerp(g[k], g[k + 1], fz[:, None, None]) if nz > 1 else g[np.zeros(D, np.int64)]
        out.append(np.ascontiguousarray(g, np.float32))
    return out
