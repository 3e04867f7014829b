"""The shape sums of labelled bodies (include/f3d.h, f3d_label_shape_sums) and the solve from them (include/f3d_host.h,
f3d_label_shape_solve) restated in numpy and Python integers: the reference of tests/test_label_shape_cpu.py and
tests/test_gpu_shape_of_labels.py.  Volumes are [z, y, x]; a direction is (dx, dy, dz)."""
import math

import numpy as np

DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1),
              (1, -1, 1), (1, -1, -1)]
SQUARES = [((1, 0, 0), (0, 1, 0)), ((1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1))]           # xy, xz, yz
S2 = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]                                        # xx yy zz xy xz yz
SUMS_DTYPE = np.dtype([("n", "<u8"), ("lo", "<i8", 3), ("hi", "<i8", 3), ("s1", "<u8", 3), ("s2", "<u8", 6), ("pairs", "<u8", 13),
                       ("squares", "<u8", 3), ("cubes", "<u8"), ("border", "<u8", 3)])
# as the header gives them: axes, face diagonals, body diagonals
WEIGHTS = (0.0915557824, 0.0739612557, 0.0703912796)
OK, EMPTY = 0, 1


def _all_equal(lab, valid, offsets):
    """the labels of the voxels p with p + o in the box for every offset o and label(p + o) == label(p), a body's"""
    d, h, w = lab.shape
    lo = [min(0, *(o[a] for o in offsets)) for a in range(3)]
    hi = [max(0, *(o[a] for o in offsets)) for a in range(3)]
    n = (w, h, d)
    if any(n[a] - hi[a] + lo[a] <= 0 for a in range(3)):
        return np.zeros(0, lab.dtype)
    base = tuple(slice(-lo[a], n[a] - hi[a]) for a in (2, 1, 0))
    a = lab[base]
    keep = valid[base].copy()
    for o in offsets:
        moved = tuple(slice(-lo[k] + o[k], n[k] - hi[k] + o[k]) for k in (2, 1, 0))
        keep &= lab[moved] == a
    return a[keep]


def label_shape_sums(labels, n_labels):
    """(sums, info): a structured array of SUMS_DTYPE with n_labels rows, and the dict of f3d_label_shape_info"""
    lab = np.asarray(labels).astype(np.int64)
    d, h, w = lab.shape
    valid = (lab >= 1) & (lab <= n_labels)
    info = dict(background=int((lab == 0).sum()), foreign=int(((lab < 0) | (lab > n_labels)).sum()), labelled=int(valid.sum()))
    count = lambda which: np.bincount(which, minlength=n_labels + 1)[1:n_labels + 1].astype(np.uint64)
    out = np.zeros(n_labels, SUMS_DTYPE)
    out["hi"] = -1
    z, y, x = np.nonzero(valid)
    of = lab[valid]
    out["n"] = count(of)
    coords = (x.astype(np.int64), y.astype(np.int64), z.astype(np.int64))
    dims = (w, h, d)
    for a in range(3):
        lo = np.full(n_labels + 1, np.iinfo(np.int64).max)
        hi = np.full(n_labels + 1, -1, np.int64)
        np.minimum.at(lo, of, coords[a])
        np.maximum.at(hi, of, coords[a])
        lo[hi < 0] = 0
        out["lo"][:, a], out["hi"][:, a] = lo[1:], hi[1:]
        s1 = np.zeros(n_labels + 1, np.int64)
        np.add.at(s1, of, coords[a])
        out["s1"][:, a] = s1[1:]
        edge = (coords[a] == 0).astype(np.int64) + (coords[a] == dims[a] - 1)
        border = np.zeros(n_labels + 1, np.int64)
        np.add.at(border, of, edge)
        out["border"][:, a] = border[1:]
    for j, (a, b) in enumerate(S2):
        s2 = np.zeros(n_labels + 1, np.int64)
        np.add.at(s2, of, coords[a] * coords[b])
        out["s2"][:, j] = s2[1:]
    for k, dk in enumerate(DIRECTIONS):
        out["pairs"][:, k] = count(_all_equal(lab, valid, [dk]))
    for k, (e, f) in enumerate(SQUARES):
        out["squares"][:, k] = count(_all_equal(lab, valid, [e, f, tuple(p + q for p, q in zip(e, f))]))
    corners = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)][1:]
    out["cubes"] = count(_all_equal(lab, valid, corners))
    return out, info


def label_shape_sums_loops(labels, n_labels):
    """the same from the words of the header, voxel by voxel in Python integers"""
    lab = np.asarray(labels)
    d, h, w = lab.shape
    dims = (w, h, d)
    rows = [dict(n=0, lo=[0, 0, 0], hi=[-1, -1, -1], s1=[0] * 3, s2=[0] * 6, pairs=[0] * 13, squares=[0] * 3, cubes=0, border=[0] * 3)
            for _ in range(n_labels)]
    info = dict(background=0, foreign=0, labelled=0)

    def at(p):
        return int(lab[p[2], p[1], p[0]]) if all(0 <= p[a] < dims[a] for a in range(3)) else None

    def add(p, o):
        return tuple(p[a] + o[a] for a in range(3))

    for z in range(d):
        for y in range(h):
            for x in range(w):
                p = (x, y, z)
                L = at(p)
                if L == 0:
                    info["background"] += 1
                    continue
                if L < 0 or L > n_labels:
                    info["foreign"] += 1
                    continue
                info["labelled"] += 1
                r = rows[L - 1]
                for a in range(3):
                    r["lo"][a] = p[a] if r["n"] == 0 else min(r["lo"][a], p[a])
                    r["hi"][a] = max(r["hi"][a], p[a])
                    r["s1"][a] += p[a]
                    r["border"][a] += (p[a] == 0) + (p[a] == dims[a] - 1)
                r["n"] += 1
                for j, (a, b) in enumerate(S2):
                    r["s2"][j] += p[a] * p[b]
                for k, dk in enumerate(DIRECTIONS):
                    r["pairs"][k] += at(add(p, dk)) == L
                for k, (e, f) in enumerate(SQUARES):
                    r["squares"][k] += all(at(add(p, o)) == L for o in (e, f, add(e, f)))
                r["cubes"] += all(at(add(p, (i, j, k))) == L for i in (0, 1) for j in (0, 1) for k in (0, 1))
    return rows, info


def as_rows(sums):
    """a structured array of sums as the list of dicts of Python integers label_shape_sums_loops gives"""
    return [{name: (sums[name][i].tolist() if sums[name].ndim > 1 else int(sums[name][i])) for name in SUMS_DTYPE.names}
            for i in range(len(sums))]


def covariance(row):
    """the covariance of a body as a union of unit cubes from a row of sums, 3 x 3: exact integers, converted once"""
    n = int(row["n"])
    s1, s2 = [int(v) for v in row["s1"]], [int(v) for v in row["s2"]]
    c = np.zeros((3, 3))
    for j, (a, b) in enumerate(S2):
        c[a, b] = c[b, a] = float(n * s2[j] - s1[a] * s1[b]) / (float(n) * float(n))
    return c + np.eye(3) / 12.0


def euler(row):
    return int(row["n"]) - sum(int(v) for v in row["pairs"][:3]) + sum(int(v) for v in row["squares"]) - int(row["cubes"])


def faces(row):
    return sum(2 * (int(row["n"]) - int(row["pairs"][k])) for k in range(3))


def surface(row, weights=WEIGHTS):
    n = int(row["n"])
    total = 0.0
    for k, dk in enumerate(DIRECTIONS):
        order = sum(abs(c) for c in dk)                              # 1, 2, 3: axis, face diagonal, body diagonal
        total += weights[order - 1] * float(2 * (n - int(row["pairs"][k]))) / math.sqrt(order)
    return 2.0 * total


def sphericity(row):
    n = float(int(row["n"]))
    return (math.pi * (6.0 * n) ** 2) ** (1.0 / 3.0) / surface(row)


def sphere_shares():
    """The share of the unit sphere nearest to +-d among the 26 directions to the neighbours, for an axis, a face diagonal and a body
    diagonal, in closed form: the cell of a direction u is the sphere inside the cone {x : x . (u - u') >= 0 for every other u'}; its
    corners are the rays where two of those planes meet inside all the others, and its area is the sum of the interior angles of that
    spherical polygon minus (m - 2) pi (Girard)."""
    units = [np.array(v, float) / math.sqrt(sum(c * c for c in v))
             for v in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)] if any(v)]
    shares = []
    for d in ((1, 0, 0), (1, 1, 0), (1, 1, 1)):
        u = np.array(d, float) / math.sqrt(sum(c * c for c in d))
        normals = [u - other for other in units if not np.allclose(other, u)]
        corners = []
        for i in range(len(normals)):
            for j in range(i + 1, len(normals)):
                ray = np.cross(normals[i], normals[j])
                if np.linalg.norm(ray) < 1e-12:
                    continue
                ray /= np.linalg.norm(ray)
                for r in (ray, -ray):
                    if all(r @ m >= -1e-12 for m in normals) and not any(np.allclose(r, c, atol=1e-9) for c in corners):
                        corners.append(r)
        # in order round u
        e1 = np.cross(u, [0.3, 0.5, 0.81])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(u, e1)
        corners.sort(key=lambda c: math.atan2(c @ e2, c @ e1))
        m = len(corners)
        angles = 0.0
        for k in range(m):
            v, before, after = corners[k], corners[k - 1], corners[(k + 1) % m]
            t1 = before - (before @ v) * v
            t2 = after - (after @ v) * v
            angles += math.acos(np.clip(t1 @ t2 / (np.linalg.norm(t1) * np.linalg.norm(t2)), -1.0, 1.0))
        area = angles - (m - 2) * math.pi
        shares.append(2.0 * area / (4.0 * math.pi))               # the cells of +d and -d
    return tuple(shares)


# ---- volumes --------------------------------------------------------------------------------------------------------------------------------

def grid(n=48):
    """z, y, x of an n^3 grid about its centre (n - 1) / 2"""
    c = (n - 1) / 2.0
    return np.meshgrid(np.arange(n) - c, np.arange(n) - c, np.arange(n) - c, indexing="ij")


def ball(radius, n=48):
    z, y, x = grid(n)
    return (x * x + y * y + z * z <= radius * radius).astype(np.int32)


def torus(big, small, n=48):
    z, y, x = grid(n)
    return ((np.sqrt(x * x + y * y) - big) ** 2 + z * z <= small * small).astype(np.int32)


# ---- the cases of the GPU tests, computed by a child interpreter -------------------------------------------------------------------------
# The restatement frees dozens of arrays of 0.66 MB per case.  In the process of the GPU tests that moves glibc's heap under the volumes
# that tests/test_gpu_pipeline.py page-locks later in the same process (LABBOOK.md), so the GPU tests get their cases from a child and
# read them as read-only file mappings, as those of nearest_ref.py and histogram_ref.py do.

def case_volume(dims, layout):
    """(labels [d, h, w] int32, n_labels) of a layout of tests/test_gpu_shape_of_labels.py"""
    from test_gpu_label_motion import label_volume
    w, h, d = dims
    if layout == "checker":
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        return (1 + (x + y + z) % 2).astype(np.int32), 2
    if layout == "cross":                                    # body 41 runs through the centre along every axis to all six box faces
        lab, _ = label_volume(dims, "voronoi")
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        mid = (x == w // 2).astype(int) + (y == h // 2) + (z == d // 2)
        lab[mid >= 2] = 41
        return lab, 41
    return label_volume(dims, layout)


def case_table(dims, layout):
    """({labels, container, sums}, info with n_labels): the container is three columns, two rows and a plane larger than the box and its
    padding carries the label of the box's far corner when that is a body's, else 1"""
    labels, n_labels = case_volume(tuple(dims), layout)
    sums, info = label_shape_sums(labels, n_labels)
    d, h, w = labels.shape
    corner = int(labels[-1, -1, -1])
    container = np.full((d + 1, h + 2, w + 3), corner if 1 <= corner <= n_labels else 1, np.int32)
    container[:d, :h, :w] = labels
    return dict(labels=labels, container=container, sums=sums), dict(info, n_labels=n_labels)


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
    subprocess.run([sys.executable, os.path.join(here, "label_shape_ref.py"), directory], check=True, cwd=here, timeout=600)
    with open(os.path.join(directory, "infos.json")) as f:
        infos = json.load(f)
    return [({name: np.load(os.path.join(directory, f"{i}_{name}.npy"), mmap_mode="r") for name in names}, info)
            for i, (names, info) in enumerate(infos)]


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
