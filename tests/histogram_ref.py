"""The numpy restatement of f3d_histogram, f3d_value_range (include/f3d.h) and of f3d_histogram_edge, f3d_otsu and f3d_histogram_rank
(include/f3d_host.h): the reference of tests/test_histogram_cpu.py and tests/test_gpu_segment_histogram.py.  Everything float is float32 with
one rounding per operation (numpy's float32 arithmetic), the Otsu objective is Python's binary64 with one rounding per operation, and
everything else is an integer."""
import numpy as np

F32 = np.float32
HISTOGRAM_INFO = ("masked", "nan", "below", "above", "used")
RANGE_INFO = ("masked", "nan", "infinite", "finite")
OTSU_OK, OTSU_DEGENERATE = 0, 1
MAX_BINS = 4096


def scale_of(lo, hi, bins):
    """scale = (float)bins / (hi - lo), both operations in float32"""
    return F32(bins) / (F32(hi) - F32(lo))


def bin_of(values, lo, hi, bins):
    """the bin of every value of a float32 array that lies in [lo, hi]: min((int)((s - lo) * scale), bins - 1)"""
    values = np.asarray(values, F32)
    offset = values - F32(lo)                                          # rounded to float32
    scaled = offset * scale_of(lo, hi, bins)                           # rounded to float32
    assert offset.dtype == F32 and scaled.dtype == F32
    return np.minimum(scaled.astype(np.int64), bins - 1)               # the conversion truncates (the values are not negative)


def histogram(volume, lo, hi, bins, mask=None):
    """(counts uint64 [bins], info dict) of a [z, y, x] float32 volume; mask: an integer volume, 0 leaves the voxel out"""
    v = np.asarray(volume, F32).ravel()
    lo, hi = F32(lo), F32(hi)
    assert np.isfinite(lo) and np.isfinite(hi) and lo < hi and 1 <= bins <= MAX_BINS
    left = np.ones(v.shape, bool) if mask is None else np.asarray(mask).ravel() != 0
    masked = ~left
    nan = left & np.isnan(v)
    with np.errstate(invalid="ignore"):
        below = left & ~nan & (v < lo)
        above = left & ~nan & ~below & (v > hi)
    used = left & ~nan & ~below & ~above
    counts = np.bincount(bin_of(v[used], lo, hi, bins), minlength=bins).astype(np.uint64)
    info = dict(masked=int(masked.sum()), nan=int(nan.sum()), below=int(below.sum()), above=int(above.sum()), used=int(used.sum()))
    assert sum(info.values()) == v.size and int(counts.sum()) == info["used"]
    return counts, info


def key_of(values):
    """the totally ordered unsigned key of the bits of float32 values: -0.0 directly below +0.0, denormals in their place"""
    bits = np.ascontiguousarray(values, F32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def float_of_key(keys):
    keys = np.asarray(keys, np.uint32)
    return np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7FFFFFFF), ~keys).astype(np.uint32).view(F32)


def value_range(volume, mask=None):
    """(min, max, info): the smallest and largest finite value by key; +inf and -inf without a finite voxel"""
    v = np.asarray(volume, F32).ravel()
    left = np.ones(v.shape, bool) if mask is None else np.asarray(mask).ravel() != 0
    nan = left & np.isnan(v)
    infinite = left & np.isinf(v)
    finite = left & np.isfinite(v)
    info = dict(masked=int((~left).sum()), nan=int(nan.sum()), infinite=int(infinite.sum()), finite=int(finite.sum()))
    if not info["finite"]:
        return F32(np.inf), F32(-np.inf), info
    keys = key_of(v[finite])
    return float_of_key(keys.min())[()], float_of_key(keys.max())[()], info


def edge(lo, hi, bins, k):
    """the smallest float32 in [lo, hi] whose bin is at least k, by bisection over the keys"""
    assert 0 <= k < bins
    if k == 0:
        return F32(lo)
    below, above = int(key_of(F32(lo)).ravel()[0]), int(key_of(F32(hi)).ravel()[0])
    while above - below > 1:
        middle = (below + above) // 2
        if int(bin_of(float_of_key(np.uint32(middle)), lo, hi, bins)) >= k:
            above = middle
        else:
            below = middle
    return float_of_key(np.uint32(above))[()]


def otsu_objective(counts, cuts):
    """the binary64 objective of a candidate, None when a class is empty: sum over the classes, left to right, of M * M / N"""
    counts = [int(c) for c in counts]
    bounds = [0] + [int(c) for c in cuts] + [len(counts)]
    total = None
    for a, b in zip(bounds[:-1], bounds[1:]):
        n = sum(counts[a:b])
        m = sum(i * counts[i] for i in range(a, b))
        if n == 0:
            return None
        md = float(m)
        term = (md * md) / float(n)
        total = term if total is None else total + term
    return total


def otsu(counts, classes):
    """(status, cuts, populations, objective): candidates in lexicographic order, replaced on strict > only"""
    counts = [int(c) for c in counts]
    bins = len(counts)
    n = np.concatenate([[0], np.cumsum(np.array(counts, dtype=object))]).tolist()
    m = np.concatenate([[0], np.cumsum(np.array([i * c for i, c in enumerate(counts)], dtype=object))]).tolist()
    if sum(c != 0 for c in counts) < classes:
        return OTSU_DEGENERATE, [], [0] * classes, 0.0

    def term(a, b):
        md = float(m[b] - m[a])
        return (md * md) / float(n[b] - n[a])

    best, best_cuts = None, None
    if classes == 2:
        for c in range(1, bins):
            if n[c] == 0 or n[bins] == n[c]:
                continue
            value = term(0, c) + term(c, bins)
            if best is None or value > best:
                best, best_cuts = value, [c]
    else:
        for c1 in range(1, bins - 1):
            if n[c1] == 0:
                continue
            first = term(0, c1)
            for c2 in range(c1 + 1, bins):
                if n[c2] == n[c1] or n[bins] == n[c2]:
                    continue
                value = (first + term(c1, c2)) + term(c2, bins)
                if best is None or value > best:
                    best, best_cuts = value, [c1, c2]
    bounds = [0] + best_cuts + [bins]
    return OTSU_OK, best_cuts, [n[b] - n[a] for a, b in zip(bounds[:-1], bounds[1:])], best


def rank(counts, r):
    """the bin of the r-th smallest counted voxel (0-based)"""
    total = 0
    for b, c in enumerate(counts):
        total += int(c)
        if total > r:
            return b
    raise ValueError("r is not below the number of counted voxels")


# ---- the layouts of the GPU tests -------------------------------------------------------------------------------------------------------

LAYOUTS = ("constant", "alternating", "ramp", "noise", "noise-3", "nan")


def layout_volume(layout, shape, seed=7):
    """a [d, h, w] float32 volume with values in [0.25, 0.75] (or all NaN): the cases the kernel's run merging meets"""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    if layout == "constant":
        v = np.full(shape, 0.5, F32)
    elif layout == "alternating":
        v = np.where(np.arange(w) % 2 == 0, F32(0.3), F32(0.7)) * np.ones(shape, F32)
    elif layout == "ramp":
        v = (F32(0.25) + F32(0.5) * (np.arange(w, dtype=F32) / F32(max(w - 1, 1)))) * np.ones(shape, F32)
    elif layout == "noise":
        v = F32(0.25) + F32(0.5) * rng.random(shape, dtype=F32)
    elif layout == "noise-3":
        v = rng.choice(np.array([0.25, 0.5, 0.75], F32), size=shape)
    elif layout == "nan":
        v = np.full(shape, np.nan, F32)
    else:
        raise ValueError(layout)
    return np.ascontiguousarray(v, F32)


def frame_volume(shape):
    """tests/golden/inputs_128.npz frame 0 (uint8 values as float32), tiled where the shape is wider, cropped to [d, h, w]"""
    import os
    frame = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs_128.npz"))["frame_0"]
    d, h, w = shape
    tiled = np.tile(frame, (-(-d // frame.shape[0]), -(-h // frame.shape[1]), -(-w // frame.shape[2])))[:d, :h, :w]
    return np.ascontiguousarray(tiled, F32)


def masks(shape, seed=11):
    """name -> mask (int32 [d, h, w]) or None: none, all zero, a half box, negative values that let voxels through"""
    d, h, w = shape
    half = np.zeros(shape, np.int32)
    half[:, :, : (w + 1) // 2] = 1
    negative = np.random.default_rng(seed).integers(-3, 2, size=shape).astype(np.int32)
    return {"none": None, "zero": np.zeros(shape, np.int32), "half": half, "negative": negative}


# ---- the cases of tests/test_gpu_segment_histogram.py, computed in a child interpreter ---------------------------------------------------------------
# The restatement builds and frees blocks of many megabytes at the large shape.  In a process with a device open that is not harmless:
# freed mapped blocks raise glibc's mmap threshold, later arrays come from the shared heap, and the page-locked volumes of
# tests/test_gpu_pipeline.py have lost their mapping on the device after such runs (LABBOOK.md).  So the GPU tests have a child
# interpreter compute their table once per module and read volumes, masks and counts as read-only file mappings: in_child() below.

TABLE_BINS = (1, 2, 64, 256, 1000, 4096)
LARGE = (160, 96, 72)                                                 # (w, h, d): there only two masks and two bin counts


def table_plan(dims):
    """(mask names, bin counts) of the table test at (w, h, d)"""
    return (("none", "negative"), (64, 4096)) if tuple(dims) == LARGE else (("none", "zero", "half", "negative"), TABLE_BINS)


def table_range(layout):
    """(lo, hi, the byte that fills the padding of the source container: 0x3F3F3F3F is 0.747 and 0x42424242 is 48.6, both inside)"""
    return (0.0, 255.0, 0x42) if layout == "frame" else (0.25, 0.75, 0x3F)


def case_table(w, h, d, layout):
    """arrays: the volume, the masks, the counts per mask and bin count; info: the counters per mask and bin count, and per mask the
    range as (bits of min, bits of max, counters)"""
    shape = (d, h, w)
    volume = frame_volume(shape) if layout == "frame" else layout_volume(layout, shape)
    lo, hi, _ = table_range(layout)
    names, bin_counts = table_plan((w, h, d))
    arrays, info = {"volume": volume}, {}
    every = masks(shape)
    for name in names:
        mask = every[name]
        if mask is not None:
            arrays[f"mask_{name}"] = mask
        low, high, counters = value_range(volume, mask)
        info[f"range_{name}"] = [int(F32(low).view(np.uint32)), int(F32(high).view(np.uint32)), counters]
        for bins in bin_counts:
            arrays[f"counts_{name}_{bins}"], info[f"info_{name}_{bins}"] = histogram(volume, lo, hi, bins, mask)
    return arrays, info


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
    subprocess.run([sys.executable, os.path.join(here, "histogram_ref.py"), directory], check=True, cwd=here, timeout=600)
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
