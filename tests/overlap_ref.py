"""The overlap of two label volumes through a displacement (include/f3d.h, f3d_label_overlap), the relabelling (f3d_relabel_labels) and
the solve from the overlap rows to the tracks (include/f3d_host.h, f3d_overlap_solve) restated in numpy and Python integers: the
reference of tests/test_overlap_cpu.py and tests/test_gpu_track_overlap.py.  Volumes are [z, y, x]."""
import numpy as np

F32 = np.float32
ROWS_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<u8"), ("ca2", "<i8", 3), ("cb2", "<i8", 3)])
TRACK_A_DTYPE = np.dtype([("n", "<u8"), ("n_lost", "<u8"), ("n_background", "<u8"), ("n_best", "<u8"), ("best_b", "<i4"),
                          ("n_targets", "<i4"), ("fraction", "<f8"), ("shift", "<f8", 3), ("iou", "<f8"), ("status", "<u4"), ("pad", "<u4")])
TRACK_B_DTYPE = np.dtype([("m", "<u8"), ("n_unreached", "<u8"), ("n_best", "<u8"), ("best_a", "<i4"), ("n_sources", "<i4"),
                          ("status", "<u4"), ("pad", "<u4")])
CLASSES = ("foreign_a", "lost_background", "lost_body", "foreign_b", "background", "overlap")
EMPTY, MATCHED, SPLIT, VANISHED, LEFT, MERGED, APPEARED = 1, 2, 4, 8, 16, 32, 64


# ---- the overlap ----------------------------------------------------------------------------------------------------------------------------

def landing(shape, u, v, w):
    """(inside [d, h, w] bool, (yx, yy, yz) int64): where every voxel lands, in the header's float32 operations; u, v, w None is the
    identity"""
    d, h, wd = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(wd), indexing="ij")
    if u is None:
        return np.ones(shape, bool), (x.astype(np.int64), y.astype(np.int64), z.astype(np.int64))
    inside = np.ones(shape, bool)
    at = []
    with np.errstate(invalid="ignore", over="ignore"):
        for grid, disp, n in ((x, u, wd), (y, v, h), (z, w, d)):
            p = grid.astype(F32) + np.asarray(disp, F32)                    # one float32 add
            assert p.dtype == F32
            inside &= ~(np.isnan(p) | (p < F32(0)) | (p > F32(n - 1)))
            q = np.floor(p + F32(0.5))                                       # float32 add, then the floor
            assert q.dtype == F32
            at.append(np.minimum(n - 1, np.where(inside, q, 0).astype(np.int64)))
    return inside, tuple(at)


def label_overlap(labels_a, n_a, labels_b, n_b, u=None, v=None, w=None):
    """(rows, info): a structured array of ROWS_DTYPE sorted by (a, b), and the dict of f3d_overlap_info of a call with room enough"""
    la, lb = np.asarray(labels_a).astype(np.int64), np.asarray(labels_b).astype(np.int64)
    assert la.shape == lb.shape and la.ndim == 3
    d, h, wd = la.shape
    dims = (wd, h, d)
    inside, (yx, yy, yz) = landing(la.shape, u, v, w)
    foreign_a = (la < 0) | (la > n_a)
    lost = ~foreign_a & ~inside
    landed = ~foreign_a & inside
    b = np.where(landed, lb[yz, yy, yx], 0)
    foreign_b = landed & ((b < 0) | (b > n_b))
    background = landed & ~foreign_b & (la == 0) & (b == 0)
    overlap = landed & ~foreign_b & ~background
    info = dict(foreign_a=int(foreign_a.sum()), lost_background=int((lost & (la == 0)).sum()), lost_body=int((lost & (la != 0)).sum()),
                foreign_b=int(foreign_b.sum()), background=int(background.sum()), overlap=int(overlap.sum()), table_lost=0)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(wd), indexing="ij")
    keyed = overlap | (lost & (la != 0))
    ka = la[keyed]
    kb = np.where(overlap, b, -1)[keyed]
    code, index = np.unique(ka * (n_b + 2) + (kb + 1), return_inverse=True)
    rows = np.zeros(len(code), ROWS_DTYPE)
    rows["a"], rows["b"] = code // (n_b + 2), code % (n_b + 2) - 1
    n = np.zeros(len(code), np.int64)
    np.add.at(n, index, 1)
    rows["n"] = n
    here = overlap[keyed]
    for j, (src, dst) in enumerate(((x, yx), (y, yy), (z, yz))):
        ca = np.zeros(len(code), np.int64)
        np.add.at(ca, index, 2 * src[keyed] - (dims[j] - 1))
        cb = np.zeros(len(code), np.int64)
        np.add.at(cb, index, np.where(here, 2 * dst[keyed] - (dims[j] - 1), 0))
        rows["ca2"][:, j], rows["cb2"][:, j] = ca, cb
    info.update(n_pairs=len(rows), complete=1)
    return rows, info


def label_overlap_loops(labels_a, n_a, labels_b, n_b, u=None, v=None, w=None):
    """the same from the words of the header, voxel by voxel: ({(a, b): [n, ca2, cb2]} in Python integers, info)"""
    la, lb = np.asarray(labels_a), np.asarray(labels_b)
    d, h, wd = la.shape
    dims = (wd, h, d)
    info = {name: 0 for name in CLASSES}
    table = {}
    for z in range(d):
        for y in range(h):
            for x in range(wd):
                a = int(la[z, y, x])
                if a < 0 or a > n_a:
                    info["foreign_a"] += 1
                    continue
                src = (x, y, z)
                if u is None:
                    p = [F32(c) for c in src]
                else:
                    p = [F32(c) + F32(f[z, y, x]) for c, f in zip(src, (u, v, w))]
                lost = any(np.isnan(q) or q < F32(0) or q > F32(n - 1) for q, n in zip(p, dims))
                if lost:
                    info["lost_background" if a == 0 else "lost_body"] += 1
                    if a == 0:
                        continue
                    key, dst = (a, -1), None
                else:
                    dst = [min(n - 1, int(np.floor(q + F32(0.5)))) for q, n in zip(p, dims)]
                    b = int(lb[dst[2], dst[1], dst[0]])
                    if b < 0 or b > n_b:
                        info["foreign_b"] += 1
                        continue
                    if a == 0 and b == 0:
                        info["background"] += 1
                        continue
                    info["overlap"] += 1
                    key = (a, b)
                row = table.setdefault(key, [0, [0, 0, 0], [0, 0, 0]])
                row[0] += 1
                for j in range(3):
                    row[1][j] += 2 * src[j] - (dims[j] - 1)
                    if dst is not None:
                        row[2][j] += 2 * dst[j] - (dims[j] - 1)
    info.update(table_lost=0, n_pairs=len(table), complete=1)
    return table, info


def as_table(rows):
    """rows of ROWS_DTYPE as the dict label_overlap_loops gives"""
    return {(int(r["a"]), int(r["b"])): [int(r["n"]), [int(c) for c in r["ca2"]], [int(c) for c in r["cb2"]]] for r in rows}


def rows_of(table):
    """the other way round, sorted by (a, b)"""
    rows = np.zeros(len(table), ROWS_DTYPE)
    for i, key in enumerate(sorted(table)):
        n, ca2, cb2 = table[key]
        rows[i] = (key[0], key[1], n, ca2, cb2)
    return rows


def relabel(labels, mapping):
    """(out int32, foreign): f3d_relabel_labels"""
    lab = np.asarray(labels).astype(np.int64)
    mapping = np.asarray(mapping, np.int64)
    n = len(mapping)
    body = (lab >= 1) & (lab <= n)
    out = np.zeros(lab.shape, np.int32)
    out[body] = mapping[lab[body] - 1]
    return out, int(((lab < 0) | (lab > n)).sum())


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------

def counts(part, min_fraction, whole):
    return float(part) >= min_fraction * float(whole)


def solve(rows, n_a, n_b, min_fraction=0.1):
    """(a of TRACK_A_DTYPE, b of TRACK_B_DTYPE, map_b int32, summary dict) in the order of include/f3d_host.h; rows in any order"""
    nan = float("nan")
    A = [dict(n=0, n_lost=0, n_background=0, n_best=0, best_b=0, n_targets=0, fraction=nan, shift=[nan] * 3, iou=nan, status=0)
         for _ in range(n_a)]
    B = [dict(m=0, n_unreached=0, n_best=0, best_a=0, n_sources=0, status=0) for _ in range(n_b)]
    table = [(int(r["a"]), int(r["b"]), int(r["n"]), [int(c) for c in r["ca2"]], [int(c) for c in r["cb2"]]) for r in rows]
    for a, b, n, ca2, cb2 in table:                                          # 1. sums and best partners
        assert 0 <= a <= n_a and -1 <= b <= n_b and not (a == 0 and b <= 0)
        if a >= 1:
            t = A[a - 1]
            t["n"] += n
            if b == -1:
                t["n_lost"] += n
            if b == 0:
                t["n_background"] += n
            if b >= 1 and n > 0 and (n > t["n_best"] or (n == t["n_best"] and b < t["best_b"])):
                t["n_best"], t["best_b"] = n, b
                t["shift"] = [float(cb2[j] - ca2[j]) / (2.0 * float(n)) for j in range(3)]
        if b >= 1:
            t = B[b - 1]
            t["m"] += n
            if a == 0:
                t["n_unreached"] += n
            if a >= 1 and n > 0 and (n > t["n_best"] or (n == t["n_best"] and a < t["best_a"])):
                t["n_best"], t["best_a"] = n, a
    for a, b, n, _, _ in table:                                              # 2. the partners whose share counts
        if a >= 1 and b >= 1 and n > 0:
            A[a - 1]["n_targets"] += counts(n, min_fraction, A[a - 1]["n"])
            B[b - 1]["n_sources"] += counts(n, min_fraction, B[b - 1]["m"])
    summary = dict(matched=0, split=0, merged=0, vanished=0, appeared=0, left=0, n_ids=n_a)
    for i, t in enumerate(A):                                                # 3. status and the doubles
        if t["n"] == 0:
            t["status"] = EMPTY
            continue
        t["fraction"] = float(t["n_best"]) / float(t["n"])
        t["iou"] = 0.0
        if t["best_b"] >= 1:
            other = B[t["best_b"] - 1]
            t["iou"] = float(t["n_best"]) / float(t["n"] + other["m"] - t["n_best"])
            if other["best_a"] == i + 1:
                t["status"] |= MATCHED
        if t["n_targets"] >= 2:
            t["status"] |= SPLIT
        if t["n_targets"] == 0:
            t["status"] |= VANISHED
        if counts(t["n_lost"], min_fraction, t["n"]):
            t["status"] |= LEFT
        for name, bit in (("matched", MATCHED), ("split", SPLIT), ("vanished", VANISHED), ("left", LEFT)):
            summary[name] += bool(t["status"] & bit)
    map_b = np.zeros(n_b, np.int32)
    for i, t in enumerate(B):                                                # and 4. the new numbers
        if t["m"] == 0:
            t["status"] = EMPTY
            continue
        if t["best_a"] >= 1 and A[t["best_a"] - 1]["best_b"] == i + 1:
            t["status"] |= MATCHED
        if t["n_sources"] >= 2:
            t["status"] |= MERGED
        if t["n_sources"] == 0:
            t["status"] |= APPEARED
        summary["merged"] += bool(t["status"] & MERGED)
        summary["appeared"] += bool(t["status"] & APPEARED)
        if t["status"] & MATCHED:
            map_b[i] = t["best_a"]
        else:
            summary["n_ids"] += 1
            map_b[i] = summary["n_ids"]
    out_a, out_b = np.zeros(n_a, TRACK_A_DTYPE), np.zeros(n_b, TRACK_B_DTYPE)
    for i, t in enumerate(A):
        for name, value in t.items():
            out_a[name][i] = value
    for i, t in enumerate(B):
        for name, value in t.items():
            out_b[name][i] = value
    return out_a, out_b, map_b, summary


# ---- the cases of the GPU tests, computed by a child interpreter -------------------------------------------------------------------------
# As in label_shape_ref.py: the restatement allocates and frees many arrays, which in the process of the GPU tests moves glibc's heap
# under the volumes tests/test_gpu_pipeline.py page-locks later (LABBOOK.md), so the GPU tests get their cases from a child and read them
# as read-only file mappings.

def mix(lab, n, rng):
    """background, negative, too large and NaN-bit values over a label volume (the mix of test_gpu_label_motion.label_volume)"""
    pick = rng.random(lab.shape)
    lab[pick < 0.10] = 0
    lab[(pick >= 0.10) & (pick < 0.14)] = -3
    lab[(pick >= 0.14) & (pick < 0.18)] = n + 1
    lab[(pick >= 0.18) & (pick < 0.20)] = np.iinfo(np.int32).max
    lab[(pick >= 0.20) & (pick < 0.22)] = np.iinfo(np.int32).min
    lab[(pick >= 0.22) & (pick < 0.24)] = 0x7FC00000
    return lab


def case_labels(dims, layout):
    """(labels_a, n_a, labels_b, n_b), int32 [d, h, w]"""
    from label_motion_ref import voronoi
    w, h, d = dims
    shape = (d, h, w)
    rng = np.random.default_rng(w * 31 + h * 7 + d)
    if layout == "one":
        return np.ones(shape, np.int32), 1, np.ones(shape, np.int32), 1
    if layout == "onekey":                                                   # one key everywhere, neither label the largest
        return np.full(shape, 3, np.int32), 5, np.full(shape, 2, np.int32), 4
    if layout == "same":
        lab = voronoi(shape, 40, seed=w)
        return lab, 40, lab.copy(), 40
    if layout == "other":
        return voronoi(shape, 40, seed=w), 40, voronoi(shape, 40, seed=w + 1), 57        # spare numbers on B's side
    if layout == "random":                                                   # more keys in every tile than the LDS table has slots
        return rng.integers(1, 1001, shape).astype(np.int32), 1000, rng.integers(1, 1001, shape).astype(np.int32), 1000
    if layout == "mix":
        return mix(voronoi(shape, 40, seed=w), 40, rng), 40, mix(voronoi(shape, 40, seed=w + 1), 40, rng), 40
    if layout == "seams":   # bodies that end exactly where the 64 x 4 x 32 tiles do, and a key that changes on the last plane of a tile
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        a = (1 + x // 64 + 3 * (y // 4) + 9 * (z // 32)).astype(np.int32)
        a[z % 32 == 31] = 40
        b = (1 + (x + 1) // 64 + 3 * ((y + 1) // 4) + 9 * ((z + 1) // 32)).astype(np.int32)
        return a, 40, b, 40
    raise ValueError(layout)


DISPLACEMENTS = ("none", "zero", "shift", "smooth", "ties", "nan", "mixed", "out-x", "out+x", "out-y", "out+y", "out-z", "out+z")


def case_displacement(dims, kind):
    """(u, v, w) float32 [d, h, w], or (None, None, None)"""
    w, h, d = dims
    shape = (d, h, w)
    rng = np.random.default_rng(w * 13 + h * 5 + d + len(kind))
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    if kind == "none":
        return None, None, None
    if kind == "zero":
        return tuple(np.zeros(shape, F32) for _ in range(3))
    if kind == "shift":
        return np.full(shape, 2, F32), np.full(shape, -1, F32), np.full(shape, 3, F32)
    smooth = ((2.5 * np.sin(0.11 * y + 0.07 * z + 0.3)).astype(F32), (1.5 * np.cos(0.09 * x - 0.05 * z)).astype(F32),
              (2.0 * np.sin(0.05 * x + 0.13 * y + 1.0)).astype(F32))
    if kind == "smooth":
        return smooth
    below, above = np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, below, -below, above, -above, 1 + below, 0.0, -0.0], F32)
    if kind == "ties":                                                       # x + t is exact or rounds in the float32 add
        return tuple(rng.choice(ties, size=shape).astype(F32) for _ in range(3))
    if kind in ("nan", "mixed"):
        out = [f.copy() for f in smooth]
        pick = rng.random(shape)
        for k, f in enumerate(out):
            f[(pick >= 0.05 * k) & (pick < 0.05 * k + 0.03)] = np.nan
        out[0][(pick >= 0.20) & (pick < 0.21)] = np.inf
        out[1][(pick >= 0.21) & (pick < 0.22)] = -np.inf
        if kind == "mixed":
            for k, f in enumerate(out):
                m = (pick >= 0.3 + 0.1 * k) & (pick < 0.38 + 0.1 * k)
                f[m] = rng.choice(ties, size=int(m.sum()))
            out[2][(pick >= 0.7) & (pick < 0.72)] = 1e30
            out[2][(pick >= 0.72) & (pick < 0.74)] = -1e-40
        return tuple(out)
    axis, sign = "xyz".index(kind[4]), (-1.0 if kind[3] == "-" else 1.0)     # everything moves 3.25 voxels towards one face
    out = [np.zeros(shape, F32) for _ in range(3)]
    out[axis] = np.full(shape, sign * 3.25, F32)
    return tuple(out)


def case_table(dims, layout, kind):
    """({labels_a, labels_b, container_a, container_b, rows[, u, v, w, container_u, container_v, container_w]}, info with n_a and n_b).
    The containers are three columns, two rows and a plane larger than the volume; the padding of the label containers carries a
    body's number, that of the displacement NaN."""
    dims = tuple(dims)
    la, n_a, lb, n_b = case_labels(dims, layout)
    u, v, w = case_displacement(dims, kind)
    rows, info = label_overlap(la, n_a, lb, n_b, u, v, w)
    d, h, wd = la.shape

    def container(inner, fill, dtype):
        c = np.full((d + 1, h + 2, wd + 3), fill, dtype)
        c[:d, :h, :wd] = inner
        return c

    arrays = dict(labels_a=la, labels_b=lb, container_a=container(la, n_a, np.int32), container_b=container(lb, 1, np.int32), rows=rows)
    if u is not None:
        for name, f in zip("uvw", (u, v, w)):
            arrays[name] = f
            arrays["container_" + name] = container(f, np.nan, F32)
    return arrays, dict(info, n_a=n_a, n_b=n_b)


def in_child(jobs, directory):
    """jobs: a list of argument lists of case_table.  A child interpreter computes them all and leaves every array as a .npy file under
    `directory`; returns a list of (dict of read-only file mappings, info dict) in their order."""
    import json
    import os
    import subprocess
    import sys
    with open(os.path.join(directory, "jobs.json"), "w") as f:
        json.dump(jobs, f)
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, os.path.join(here, "overlap_ref.py"), directory], check=True, cwd=here, timeout=600)
    with open(os.path.join(directory, "infos.json")) as f:
        infos = json.load(f)

    def mapped(path):
        try:
            return np.load(path, mmap_mode="r")
        except ValueError:                                                   # nothing to map of an empty table
            return np.load(path)

    return [({name: mapped(os.path.join(directory, f"{i}_{name}.npy")) for name in names}, info) for i, (names, info) in enumerate(infos)]


if __name__ == "__main__":
    import json
    import os
    import sys
    out = sys.argv[1]
    with open(os.path.join(out, "jobs.json")) as f:
        todo = json.load(f)
    done = []
    for i, args in enumerate(todo):
        arrays, info = case_table(*args)
        for name, a in arrays.items():
            np.save(os.path.join(out, f"{i}_{name}.npy"), a)
        done.append((sorted(arrays), info))
    with open(os.path.join(out, "infos.json"), "w") as f:
        json.dump(done, f)
