"""The restatement of f3d_label_components (include/f3d.h) in plain numpy and Python, and the layouts its tests share.  Never the code
under test, and no scipy in here: tests/test_components_cpu.py checks this file against scipy.ndimage.label and against a flood fill.

label_components(volume, lo, hi, min_voxels) -> (labels int32 [d, h, w], sizes uint64 [n_labels], info dict)
  mask     float32 compares lo <= s and s <= hi (a NaN fails both)
  runs     maximal stretches of foreground along x within a row, numbered in linear order x + W (y + H z)
  union    two runs that share a +y or a +z face are joined, the larger root below the smaller: the root of a set is its first run, and
           the first voxel of that run is the smallest linear index of the component
  numbers  the components of at least min_voxels voxels, 1 .. n_labels in ascending order of that index
"""
import numpy as np

F32 = np.float32
INFO = ("foreground", "background", "nan", "n_components", "n_labels", "dropped_components", "dropped_voxels", "largest")


def foreground(volume, lo, hi):
    v = np.asarray(volume, F32)
    with np.errstate(invalid="ignore"):
        return (F32(lo) <= v) & (v <= F32(hi))


def label_components(volume, lo=-np.inf, hi=np.inf, min_voxels=1):
    v = np.asarray(volume, F32)
    assert v.ndim == 3 and v.size and min_voxels >= 1
    mask = foreground(v, lo, hi)
    d, h, w = mask.shape
    # runs along x: a run starts where a foreground voxel has no foreground voxel to its left in the row
    start = mask.copy()
    start[:, :, 1:] &= ~mask[:, :, :-1]
    run = np.cumsum(start.ravel()).reshape(mask.shape) - 1           # the run of a foreground voxel, in linear order
    n_runs = int(start.sum())
    parent = list(range(n_runs))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    pairs = []
    for a, b in ((np.s_[:, :-1, :], np.s_[:, 1:, :]), (np.s_[:-1, :, :], np.s_[1:, :, :])):
        both = mask[a] & mask[b]
        if both.any():
            pairs.append(np.unique(run[a][both].astype(np.int64) * n_runs + run[b][both]))
    for key in (np.unique(np.concatenate(pairs)).tolist() if pairs else []):
        ra, rb = find(key // n_runs), find(key % n_runs)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n_runs)], np.int64)       # of every run: the first run of its component
    size_of = np.bincount(root[run[mask]], minlength=n_runs) if n_runs else np.zeros(0, np.int64)    # voxels, at the root run
    is_root = size_of > 0
    kept = is_root & (size_of >= min_voxels)
    number = np.where(kept, np.cumsum(kept), 0)                      # runs are in linear order, so roots are too
    labels = np.zeros(mask.shape, np.int32)
    if n_runs:
        labels[mask] = number[root[run[mask]]]
    sizes = size_of[kept].astype(np.uint64)
    info = dict(foreground=int(mask.sum()), background=int(mask.size - mask.sum()), nan=int(np.isnan(v).sum()),
                n_components=int(is_root.sum()), n_labels=int(kept.sum()), dropped_components=int((is_root & ~kept).sum()),
                dropped_voxels=int(size_of[is_root & ~kept].sum()), largest=int(size_of.max()) if n_runs else 0)
    return labels, sizes, info


def flood_fill(mask, min_voxels=1):
    """the same result from a stack-based flood fill started at every voxel in linear order (small volumes): (labels, sizes)"""
    d, h, w = mask.shape
    comp = np.zeros(mask.shape, np.int64)
    sizes = []
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if not mask[z, y, x] or comp[z, y, x]:
                    continue
                sizes.append(0)
                stack = [(z, y, x)]
                comp[z, y, x] = len(sizes)
                while stack:
                    cz, cy, cx = stack.pop()
                    sizes[-1] += 1
                    for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                        nz, ny, nx = cz + dz, cy + dy, cx + dx
                        if 0 <= nz < d and 0 <= ny < h and 0 <= nx < w and mask[nz, ny, nx] and not comp[nz, ny, nx]:
                            comp[nz, ny, nx] = len(sizes)
                            stack.append((nz, ny, nx))
    sizes = np.array(sizes, np.int64)
    kept = sizes >= min_voxels
    number = np.concatenate([[0], np.where(kept, np.cumsum(kept), 0)])
    return number[comp].astype(np.int32), sizes[kept].astype(np.uint64)


# ---- layouts: boolean masks [d, h, w] ------------------------------------------------------------------------------------------------------

def grid(shape):
    d, h, w = shape
    return np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")


def checkerboard(shape):
    z, y, x = grid(shape)
    return (x + y + z) % 2 == 0


def serpentine(shape):
    """one body, a single-voxel path: in an even plane full rows at even y joined at alternating ends by one voxel at odd y; an odd plane
    holds the one voxel that leads on, alternately at the end and at the start of that pattern"""
    d, h, w = shape
    plane = np.zeros((h, w), bool)
    plane[0::2, :] = True
    for y in range(1, h, 2):
        plane[y, w - 1 if ((y - 1) // 2) % 2 == 0 else 0] = True
    last = h - 1
    if last % 2 == 0:
        end = (last, w - 1 if (last // 2) % 2 == 0 else 0)
    else:
        end = (last, w - 1 if ((last - 1) // 2) % 2 == 0 else 0)
    m = np.zeros(shape, bool)
    m[0::2] = plane
    for z in range(1, d, 2):
        at = end if ((z - 1) // 2) % 2 == 0 else (0, 0)
        m[z, at[0], at[1]] = True
    return m


def comb(shape, axis):
    """U-shaped bodies whose two arms run along `axis` (0: z, 1: y, 2: x) and join only at its highest index"""
    z, y, x = grid(shape)
    d, h, w = shape
    if axis == 2:
        return (z % 2 == 0) & ((y % 4 == 0) | (y % 4 == 2) | ((y % 4 == 1) & (x == w - 1)))
    if axis == 1:
        return (z % 2 == 0) & ((x % 4 == 0) | (x % 4 == 2) | ((x % 4 == 1) & (y == h - 1)))
    return (y % 2 == 0) & ((x % 4 == 0) | (x % 4 == 2) | ((x % 4 == 1) & (z == d - 1)))


def noise(shape, p, seed=0):
    return np.random.default_rng(seed).random(shape) < p


def without_walls(labels):
    """the cells of a label volume with every voxel that differs from its +x, +y or +z neighbour set to background"""
    wall = np.zeros(labels.shape, bool)
    wall[:, :, :-1] |= labels[:, :, :-1] != labels[:, :, 1:]
    wall[:, :-1, :] |= labels[:, :-1, :] != labels[:, 1:, :]
    wall[:-1, :, :] |= labels[:-1, :, :] != labels[1:, :, :]
    return ~wall


def diagonal(shape):
    """voxels that meet others only across an edge ((0,0,0) and (1,1,0) of every 4^3 cell) or a corner ((3,3,3) and the next cell's (0,0,0))"""
    z, y, x = grid(shape)
    a = (x % 4 == 0) & (y % 4 == 0) & (z % 4 == 0)
    b = (x % 4 == 1) & (y % 4 == 1) & (z % 4 == 0)
    c = (x % 4 == 3) & (y % 4 == 3) & (z % 4 == 3)
    return a | b | c


def bricks(shape, brick):
    """bricks of brick = (bz, by, bx) voxels, walls included: the last voxel of every period along every axis is background.  Returns
    (mask, labels, sizes) in closed form: the roots ascend with (iz, iy, ix), so brick (ix, iy, iz) is 1 + ix + nx (iy + ny iz)"""
    z, y, x = grid(shape)
    bz, by, bx = brick
    mask = (x % bx != bx - 1) & (y % by != by - 1) & (z % bz != bz - 1)
    extent = lambda n, b: np.array([min(b - 1, n - i * b) for i in range(-(-n // b)) if n - i * b > 0])
    ez, ey, ex = extent(shape[0], bz), extent(shape[1], by), extent(shape[2], bx)
    ez, ey, ex = ez[ez > 0], ey[ey > 0], ex[ex > 0]
    labels = np.where(mask, 1 + x // bx + len(ex) * (y // by + len(ey) * (z // bz)), 0).astype(np.int32)
    sizes = (ez[:, None, None] * ey[None, :, None] * ex[None, None, :]).ravel().astype(np.uint64)
    return mask, labels, sizes


def as_volume(mask, inside=1.0, outside=0.0):
    return np.where(mask, F32(inside), F32(outside)).astype(F32)


LAYOUTS = ("empty", "full", "checker", "serpentine", "serpentine-mirrored", "comb-x", "comb-y", "comb-z", "noise-0.31", "noise-0.6",
           "voronoi", "diagonal")


def layout_mask(name, shape):
    """the mask [d, h, w] of one of LAYOUTS"""
    if name == "empty":
        return np.zeros(shape, bool)
    if name == "full":
        return np.ones(shape, bool)
    if name == "checker":
        return checkerboard(shape)
    if name == "serpentine":
        return serpentine(shape)
    if name == "serpentine-mirrored":
        return serpentine(shape)[::-1, ::-1, ::-1].copy()
    if name.startswith("comb-"):
        return comb(shape, {"x": 2, "y": 1, "z": 0}[name[-1]])
    if name.startswith("noise-"):
        return noise(shape, float(name[6:]), seed=sum(shape))
    if name == "voronoi":
        from label_motion_ref import voronoi
        return without_walls(voronoi(shape, 40, seed=3))
    if name == "diagonal":
        return diagonal(shape)
    raise ValueError(name)


def apply_min_voxels(labels, sizes, info, min_voxels):
    """(labels, sizes, info) for another min_voxels from the result for min_voxels = 1, in which every component has a number"""
    assert info["dropped_components"] == 0
    kept = sizes >= min_voxels
    number = np.concatenate([[0], np.where(kept, np.cumsum(kept), 0)])
    out = dict(info, n_labels=int(kept.sum()), dropped_components=int((~kept).sum()), dropped_voxels=int(sizes[~kept].sum()))
    return number[labels].astype(np.int32), sizes[kept].astype(np.uint64), out
