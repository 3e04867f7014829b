"""numpy restatements of f3d_nearest_seed and f3d_split_components (include/f3d.h), written from the definitions and never from the
kernels: the brute-force minimum over all seeds for small boxes, the separable three-pass form with the tie rule for larger ones (each
pass a plain argmin over the whole line, first minimum = smallest coordinate), and the split of touching bodies on top of
components_ref.  Volumes are [z, y, x]; the box index of (x, y, z) is x + W (y + H z), numpy's ravel order."""
import numpy as np

import components_ref as cref

NO_SEED_D2 = 2 ** 31 - 1
OUTPUTS = ("d2", "index", "value")
INFO = ("seeds", "d2_max", "unreached")
SPLIT_INFO = cref.INFO + ("connected_components", "core_voxels", "n_cores", "remainder_bodies", "remainder_voxels")
_BIG = np.int64(2) ** 40


def seed_mask(values, mode):
    values = np.asarray(values)
    return values != 0 if mode == "nonzero" else values == 0


def _result(values, seeds, d2, index):
    values = np.asarray(values).astype(np.int32)
    none = index < 0
    value = np.where(none, 0, values.ravel()[np.where(none, 0, index)]).astype(np.int32)
    n = int(seeds.sum())
    info = dict(seeds=n, d2_max=int(d2.max()), unreached=0 if n else int(seeds.size))
    return d2.astype(np.int32), index.astype(np.int32), value, info


def nearest_brute(values, mode="nonzero"):
    """(d2, index, value, info) by the definition: per voxel the minimum over all seeds of the squared distance, argmin over the seeds in
    raster order (numpy's argmin returns the first minimum: the smallest box index)"""
    seeds = seed_mask(values, mode)
    d, h, w = seeds.shape
    z, y, x = [a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")]
    at = np.flatnonzero(seeds.ravel())                                  # ascending box index
    if not at.size:
        return _result(values, seeds, np.full(seeds.shape, NO_SEED_D2, np.int64), np.full(seeds.shape, -1, np.int64))
    dist = (x[:, None] - x[at][None, :]) ** 2 + (y[:, None] - y[at][None, :]) ** 2 + (z[:, None] - z[at][None, :]) ** 2
    first = dist.argmin(axis=1)
    return _result(values, seeds, dist[np.arange(dist.shape[0]), first].reshape(seeds.shape), at[first].reshape(seeds.shape))


def _line_pass(cost, axis):
    """cost [z, y, x] (>= _BIG: nothing) -> (min over c' along axis of cost(c') + (c - c')^2, the smallest such c'), whole lines at once"""
    n = cost.shape[axis]
    c = np.arange(n, dtype=np.int64)
    moved = np.moveaxis(cost, axis, -1)                                  # [..., c']
    total = moved[..., None, :] + ((c[:, None] - c[None, :]) ** 2)       # [..., c, c']
    first = total.argmin(axis=-1)
    best = np.take_along_axis(total, first[..., None], axis=-1)[..., 0]
    return np.moveaxis(best, -1, axis), np.moveaxis(first, -1, axis)


def nearest_separable(values, mode="nonzero"):
    """the same through the three passes: x keeps the nearest seed of the row (the left one on a tie), y the smaller y', z the smaller z'"""
    seeds = seed_mask(values, mode)
    d, h, w = seeds.shape
    if not seeds.any():
        return _result(values, seeds, np.full(seeds.shape, NO_SEED_D2, np.int64), np.full(seeds.shape, -1, np.int64))
    gx, sx = _line_pass(np.where(seeds, np.int64(0), _BIG), 2)
    gy, sy = _line_pass(gx, 1)
    sx = np.take_along_axis(sx, sy, axis=1)                               # the row y' chosen brings its x'
    gz, sz = _line_pass(gy, 0)
    sx, sy = np.take_along_axis(sx, sz, axis=0), np.take_along_axis(sy, sz, axis=0)
    assert (gz < _BIG).all()
    return _result(values, seeds, gz, sx + w * (sy + h * sz))


def distance_squared(mask):
    """squared distance of every voxel to the nearest voxel where mask is False (NO_SEED_D2 when there is none)"""
    return nearest_separable(np.asarray(mask).astype(np.int32), "zero")[0]


def split_components(volume, lo, hi, core_d2, min_voxels=1):
    """(labels, sizes, info) of f3d_split_components, items 1 to 6 of its definition"""
    assert core_d2 >= 1 and min_voxels >= 1
    v = np.asarray(volume, cref.F32)
    fg = cref.foreground(v, lo, hi)
    comp, _, cinfo = cref.label_components(v, lo, hi, 1)                  # C: every component has a number
    d2 = distance_squared(fg)
    core = fg & (d2 >= core_d2)
    body, _, minfo = cref.label_components(cref.as_volume(core), 0.5, 1.0, 1)
    _, index, _, _ = nearest_separable(core.astype(np.int32), "nonzero")
    flat_comp, flat_body = comp.ravel().astype(np.int64), body.ravel().astype(np.int64)
    idx = index.ravel().astype(np.int64)
    has = idx >= 0
    same = has & (flat_comp[np.where(has, idx, 0)] == flat_comp)
    n_cores = minfo["n_labels"]
    key = np.where(same, flat_body[np.where(has, idx, 0)], n_cores + flat_comp)     # a core body, or the remainder of a component
    inside = fg.ravel()
    remainder = inside & ~same
    keys, first, counts = np.unique(key[inside], return_index=True, return_counts=True)
    roots = np.flatnonzero(inside)[first]                                # np.unique's first occurrence: the smallest box index
    order = np.argsort(roots)
    keys, roots, counts = keys[order], roots[order], counts[order]
    kept = counts >= min_voxels
    number = np.zeros(int(key.max()) + 1 if key.size else 1, np.int64)
    number[keys[kept]] = np.arange(1, int(kept.sum()) + 1)
    labels = np.where(inside, number[np.where(inside, key, 0)], 0).astype(np.int32).reshape(fg.shape)
    info = dict(foreground=cinfo["foreground"], background=cinfo["background"], nan=cinfo["nan"], n_components=len(keys),
                n_labels=int(kept.sum()), dropped_components=int((~kept).sum()), dropped_voxels=int(counts[~kept].sum()),
                largest=int(counts.max()) if len(counts) else 0, connected_components=cinfo["n_components"],
                core_voxels=int(core.sum()), n_cores=n_cores, remainder_bodies=int(np.unique(key[remainder]).size),
                remainder_voxels=int(remainder.sum()))
    return labels, counts[kept].astype(np.uint64), info


def sphere_packing(shape=(40, 48, 56), radius=9, pitch=16, first=8, jitter=1.5, seed=4):
    """overlapping spheres on a lattice, every centre jittered: one face-connected component that a split takes apart"""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    mask = np.zeros(shape, bool)
    count = 0
    for cz in range(first, d, pitch):
        for cy in range(first, h, pitch):
            for cx in range(first, w, pitch):
                c = np.array([cz, cy, cx]) + rng.uniform(-jitter, jitter, 3)
                mask |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= radius ** 2
                count += 1
    return mask, count


LAYOUTS = ("none", "all", "corner-0", "corner-1", "corner-2", "corner-3", "corner-4", "corner-5", "corner-6", "corner-7", "face-x0",
           "face-x1", "face-y0", "face-y1", "face-z0", "face-z1", "checker", "pair-x", "pair-y", "pair-z", "pair-diagonal", "noise-0.001",
           "noise-0.3")


def layout_mask(name, shape):
    """the seeds [d, h, w] of one of LAYOUTS"""
    d, h, w = shape
    m = np.zeros(shape, bool)
    if name == "all":
        m[:] = True
    elif name.startswith("corner-"):
        k = int(name[-1])
        m[(d - 1) * (k >> 2 & 1), (h - 1) * (k >> 1 & 1), (w - 1) * (k & 1)] = True
    elif name.startswith("face-"):
        axis, side = {"x": 2, "y": 1, "z": 0}[name[5]], int(name[6])
        index = [slice(None)] * 3
        index[axis] = -1 if side else 0
        m[tuple(index)] = True
    elif name == "checker":
        m = cref.checkerboard(shape)
    elif name.startswith("pair-"):
        # two seeds equidistant from the voxels midway between them: along one axis, and along the space diagonal
        cz, cy, cx = d // 2, h // 2, w // 2
        if name == "pair-diagonal":
            m[max(cz - 1, 0), max(cy - 1, 0), max(cx - 1, 0)] = True
            m[min(cz + 1, d - 1), min(cy + 1, h - 1), min(cx + 1, w - 1)] = True
        else:
            axis = {"x": 2, "y": 1, "z": 0}[name[5]]
            for off in (-1, 1):
                at = [cz, cy, cx]
                at[axis] = min(max(at[axis] + off, 0), shape[axis] - 1)
                m[tuple(at)] = True
    elif name.startswith("noise-"):
        m = cref.noise(shape, float(name[6:]), seed=7)
    else:
        assert name == "none", name
    return m


def necked_balls(shape=(24, 22, 44)):
    """two balls of radius 6 joined by a neck of radius 1.5, and a ball of radius 2 behind one plane of background next to the first:
    at core_d2 = 16 the two balls have a core each, the neck and the small ball have none"""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    ball = lambda cz, cy, cx, r2: (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= r2
    mask = ball(11, 10, 9, 36) | ball(11, 10, 27, 36)
    mask |= ((z - 11) ** 2 + (y - 10) ** 2 <= 2) & (x >= 9) & (x <= 27)
    small = ball(11, 10, 37, 4)                                          # x 35 .. 39; the second ball ends at x = 33: x = 34 is background
    assert not (mask & small).any() and not mask[:, :, 34].any()
    return mask | small, small


# ---- cases computed in a process of their own --------------------------------------------------------------------------------------------
# The restatements above build and free blocks of many megabytes (a whole line against itself for every line).  In the process of the
# GPU tests that is not harmless: freed mapped blocks raise glibc's mmap threshold, later arrays come from the shared heap, and the
# page-locked volumes of tests/test_gpu_pipeline.py have lost their mapping on the device after such runs (LABBOOK.md).  So the GPU tests
# have a child interpreter compute their cases once per module and read the results as file mappings: in_child() below.

def case_nearest(w, h, d, layout, mode):
    """values whose seeds, in `mode`, are the layout's voxels, and their restatement: brute force for small boxes, separable otherwise"""
    seeds = layout_mask(layout, (d, h, w))
    numbers = (np.arange(d * h * w, dtype=np.int64).reshape(d, h, w) * 2654435761 % 1000003 + 1).astype(np.int32)   # none is zero
    numbers[::2, ::3, ::2] *= -1
    values = (np.where(seeds, numbers, 0) if mode == "nonzero" else np.where(seeds, 0, numbers)).astype(np.int32)
    d2, index, value, info = nearest_brute(values, mode) if d * h * w <= 512 else nearest_separable(values, mode)
    return dict(values=values, d2=d2, index=index, value=value), info


def split_volume(name):
    """the float volumes of tests/test_gpu_split.py by name; foreground is 0.5 <= value"""
    if name in ("packing", "frames"):
        mask, count = sphere_packing()
        assert count == 18
        volume = cref.as_volume(mask, 0.75, 0.25)
        if name == "frames":                                             # a texture inside the spheres for the solver to hold on to
            z, y, x = np.meshgrid(*[np.arange(n, dtype=cref.F32) for n in volume.shape], indexing="ij")
            texture = (0.05 * np.sin(0.7 * x) * np.cos(0.5 * y + 0.3 * z)).astype(cref.F32)
            volume = (volume + np.where(mask, texture, 0)).astype(cref.F32)
        return volume
    if name == "necked":
        return cref.as_volume(necked_balls()[0], 0.75, 0.25)
    if name == "noise-nan":                                              # noise at 0.6 with NaN holes
        volume = np.where(cref.noise((33, 5, 65), 0.6, seed=2), cref.F32(0.75), cref.F32(0.25))
        volume[np.random.default_rng(5).random(volume.shape) < 0.02] = np.nan
        return volume
    assert name == "box", name
    return np.full((6, 5, 7), 0.75, cref.F32)


def case_split(name, core_d2, min_voxels):
    """a volume of split_volume, its split and, as info["contacts"], the number of contacts between the resulting bodies"""
    import contacts_ref
    volume = split_volume(name)
    labels, sizes, info = split_components(volume, 0.5, np.inf, core_d2, min_voxels)
    extra = dict(info)
    n = info["n_labels"]
    extra["contacts"] = len(contacts_ref.label_contacts(None, None, None, labels, n)[0]) if n else 0
    extra["plain_components"] = cref.label_components(volume, 0.5, np.inf, 1)[2]["n_components"]
    arrays = dict(volume=volume, labels=labels, sizes=sizes)
    if name == "necked":
        arrays["small"] = necked_balls()[1]
    return arrays, extra


CASES = {"nearest": case_nearest, "split": case_split}


def in_child(jobs, directory):
    """jobs: a list of (kind, args) with kind in CASES and args a list of numbers and strings.  A child interpreter computes them all and
    leaves every array as a .npy file under `directory`; returns a list of (dict of read-only file mappings, info dict) in their order."""
    import json
    import os
    import subprocess
    import sys
    with open(os.path.join(directory, "jobs.json"), "w") as f:
        json.dump(jobs, f)
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, os.path.join(here, "nearest_ref.py"), directory], check=True, cwd=here, timeout=600)
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
    for i, (kind, args) in enumerate(todo):
        arrays, info = CASES[kind](*args)
        for name, a in arrays.items():
            np.save(os.path.join(out, f"{i}_{name}.npy"), a)
        done.append((sorted(arrays), info))
    with open(os.path.join(out, "infos.json"), "w") as f:
        json.dump(done, f)
