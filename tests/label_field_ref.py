"""The numpy restatement of f3d_label_field_sums and f3d_paint_labels (include/f3d.h) and of f3d_label_field_solve and
f3d_label_field_shift (include/f3d_host.h): the reference of tests/test_label_field_cpu.py and tests/test_gpu_stats_of_label_field.py.
Every float32 step is numpy's float32 arithmetic with one rounding per operation, every sum a Python or int64 integer that cannot
overflow at the sizes used here (asserted), the keys are those of tests/histogram_ref.py, whose bin function is imported and not restated,
and the solve is Python's binary64 with one rounding per operation on exact Python integers."""
import math

import numpy as np

import histogram_ref as href

F32 = np.float32
INFO = ("background", "foreign", "nan", "out_of_range", "used")
SUMS_DTYPE = np.dtype([("n", "<u8"), ("min_key", "<u8"), ("max_key", "<u8"), ("iq", "<i8"), ("iqq_lo", "<u8"), ("iqq_hi", "<u8"),
                       ("below", "<u8"), ("above", "<u8")])
STAT_DTYPE = np.dtype([("status", "<i4"), ("q05_bin", "<i4"), ("median_bin", "<i4"), ("q95_bin", "<i4"), ("n", "<u8"), ("below", "<u8"),
                       ("above", "<u8"), ("min", "<f8"), ("max", "<f8"), ("mean", "<f8"), ("variance", "<f8"), ("std", "<f8"),
                       ("q05", "<f8"), ("median", "<f8"), ("q95", "<f8")])
OK, EMPTY, SMALL = 0, 1, 2
LIMIT = F32(16777216.0)
QUIET_NAN = 0x7FC00000


def quantise(values, shift):
    """(t, takes part, q) of float32 values that are not NaN: t = s * 2^shift as ONE float32 product, |t| <= 2^24, q = rint(t) to even"""
    s = np.asarray(values, F32)
    scale = F32(math.ldexp(1.0, shift))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = s * scale
    assert t.dtype == F32
    with np.errstate(invalid="ignore"):
        inside = np.abs(t) <= LIMIT
    q = np.rint(np.where(inside, t, F32(0))).astype(np.int64)
    return t, inside, q


def label_field_sums(field, labels, n_labels, shift, lo=0.0, hi=0.0, bins=0):
    """(rows SUMS_DTYPE [n_labels], counts uint32 [n_labels, bins] or None, info dict) of a [z, y, x] float32 field and int32 labels"""
    s = np.ascontiguousarray(field, F32).ravel()
    lab = np.asarray(labels).ravel().astype(np.int64)
    assert s.shape == lab.shape and -100 <= shift <= 100 and 0 <= bins <= 256 and lab.size < 2 ** 20
    background = lab == 0
    foreign = (lab < 0) | (lab > n_labels)
    body = ~background & ~foreign
    nan = body & np.isnan(s)
    _, inside, q = quantise(s, shift)
    out_of_range = body & ~nan & ~inside
    used = body & ~nan & inside
    info = dict(background=int(background.sum()), foreign=int(foreign.sum()), nan=int(nan.sum()), out_of_range=int(out_of_range.sum()),
                used=int(used.sum()))
    assert sum(info.values()) == s.size
    at = lab[used] - 1
    v, q = s[used], q[used]
    rows = np.zeros(n_labels, SUMS_DTYPE)
    rows["n"] = np.bincount(at, minlength=n_labels)
    keys = href.key_of(v).astype(np.uint64)
    low = np.full(n_labels, 0xFFFFFFFF, np.uint64)
    high = np.zeros(n_labels, np.uint64)
    np.minimum.at(low, at, keys)
    np.maximum.at(high, at, keys)
    rows["min_key"], rows["max_key"] = low, high
    iq = np.zeros(n_labels, np.int64)                                 # |q| <= 2^24 and fewer than 2^20 voxels: below 2^44
    np.add.at(iq, at, q)
    rows["iq"] = iq
    qq = q * q                                                        # <= 2^48
    part_lo, part_hi = np.zeros(n_labels, np.int64), np.zeros(n_labels, np.int64)
    np.add.at(part_lo, at, qq & 0xFFFFFFFF)                           # below 2^52
    np.add.at(part_hi, at, qq >> 32)                                  # below 2^37
    for i in range(n_labels):
        total = (int(part_hi[i]) << 32) + int(part_lo[i])
        rows["iqq_lo"][i], rows["iqq_hi"][i] = total & 0xFFFFFFFF, total >> 32
    counts = None
    if bins:
        lo, hi = F32(lo), F32(hi)
        assert np.isfinite(lo) and np.isfinite(hi) and lo < hi
        below, above = v < lo, v > hi
        rows["below"] = np.bincount(at[below], minlength=n_labels)
        rows["above"] = np.bincount(at[above], minlength=n_labels)
        binned = ~below & ~above
        flat = at[binned] * bins + href.bin_of(v[binned], lo, hi, bins)
        counts = np.bincount(flat, minlength=n_labels * bins).astype(np.uint32).reshape(n_labels, bins)
        assert np.array_equal(rows["below"] + rows["above"] + counts.sum(axis=1).astype(np.uint64), rows["n"])
    assert int(rows["n"].sum()) == info["used"]
    return rows, counts, info


def paint_labels(labels, values):
    """the bits (uint32) of f3d_paint_labels: values[l - 1] for l in 1 .. len(values), the quiet NaN elsewhere"""
    lab = np.asarray(labels).astype(np.int64)
    bits = np.ascontiguousarray(values, F32).view(np.uint32)
    body = (lab >= 1) & (lab <= len(bits))
    return np.where(body, bits[np.where(body, lab - 1, 0)], np.uint32(QUIET_NAN)).astype(np.uint32)


def shift_of(lo, hi, finite):
    """f3d_label_field_shift"""
    lo, hi = float(F32(lo)), float(F32(hi))
    if finite == 0 or not (math.isfinite(lo) and math.isfinite(hi)):
        return 0
    m = max(abs(lo), abs(hi))
    if m == 0.0:
        return 0
    return min(100, max(-100, 24 - math.frexp(m)[1]))


def rank_bin(row, r):
    """the first bin whose cumulative count exceeds r"""
    total = 0
    for k, c in enumerate(row):
        total += int(c)
        if total > r:
            return k
    raise AssertionError("r is not below the sum of the counts")


def solve(rows, counts, shift, lo=0.0, hi=0.0, bins=0, min_voxels=1):
    """(stats STAT_DTYPE [n_labels], summary dict): f3d_label_field_solve from exact Python integers"""
    nan = float("nan")
    out = np.zeros(len(rows), STAT_DTYPE)
    edges = [float(href.edge(lo, hi, bins, k)) for k in range(bins)] + [float(F32(hi))] if bins else []
    summary = dict(ok=0, empty=0, small=0, mean=nan)
    weighted, weight = 0.0, 0.0
    for i, r in enumerate(rows):
        n, iq = int(r["n"]), int(r["iq"])
        o = out[i]
        o["n"], o["below"], o["above"] = n, r["below"], r["above"]
        o["q05_bin"] = o["median_bin"] = o["q95_bin"] = -1
        o["q05"] = o["median"] = o["q95"] = nan
        if n == 0:
            o["status"] = EMPTY
            for name in ("min", "max", "mean", "variance", "std"):
                o[name] = nan
            summary["empty"] += 1
        else:
            o["status"] = SMALL if n < min_voxels else OK
            o["min"] = float(href.float_of_key(np.uint32(int(r["min_key"])))[()])
            o["max"] = float(href.float_of_key(np.uint32(int(r["max_key"])))[()])
            o["mean"] = math.ldexp(float(iq) / float(n), -shift)          # both conversions and the division rounded once each
            iqq = (int(r["iqq_hi"]) << 32) + int(r["iqq_lo"])
            v = n * iqq - iq * iq
            assert 0 <= v < 2 ** 111
            vq = float(v) / float(n) / float(n)                           # float(int) rounds to nearest, ties to even
            o["variance"] = math.ldexp(vq, -2 * shift)
            o["std"] = math.ldexp(math.sqrt(vq), -shift)
            if o["status"] == OK:
                summary["ok"] += 1
                weighted = weighted + float(n) * float(o["mean"])
                weight = weight + float(n)
            else:
                summary["small"] += 1
        if bins:
            m = int(counts[i].astype(np.uint64).sum())
            if m > 0:
                ranks = ((m - 1) // 20, (m - 1) // 2, (m - 1) - (m - 1) // 20)
                for name, rank in zip(("q05", "median", "q95"), ranks):
                    k = rank_bin(counts[i], rank)
                    o[name + "_bin"] = k
                    o[name] = (edges[k] + edges[k + 1]) / 2.0
    if summary["ok"]:
        summary["mean"] = weighted / weight
    return out, summary


def loops(field, labels, n_labels, shift, lo=0.0, hi=0.0, bins=0):
    """label_field_sums by a loop over the voxels, label by label, in Python numbers: what the vectorised restatement is held to"""
    field = np.ascontiguousarray(field, F32)
    rows = np.zeros(n_labels, SUMS_DTYPE)
    rows["min_key"] = 0xFFFFFFFF
    counts = np.zeros((n_labels, bins), np.uint32) if bins else None
    scale = F32(math.ldexp(1.0, shift))
    for L in range(1, n_labels + 1):
        n = iq = iqq = below = above = 0
        low, high = 0xFFFFFFFF, 0
        for z, y, x in zip(*np.nonzero(np.asarray(labels) == L)):
            s = field[z, y, x]
            if s != s:
                continue
            with np.errstate(over="ignore", under="ignore"):
                t = F32(s * scale)
            if not abs(t) <= LIMIT:
                continue
            q = int(np.rint(t))
            key = int(href.key_of(s).ravel()[0])
            n, iq, iqq, low, high = n + 1, iq + q, iqq + q * q, min(low, key), max(high, key)
            if bins:
                if s < F32(lo):
                    below += 1
                elif s > F32(hi):
                    above += 1
                else:
                    counts[L - 1, int(href.bin_of(s, lo, hi, bins))] += 1
        rows[L - 1] = (n, low, high, iq, iqq & 0xFFFFFFFF, iqq >> 32, below, above)
    return rows, counts


# ---- the cases of the GPU tests, computed by a child interpreter -------------------------------------------------------------------------
# As in label_shape_ref.py: the GPU tests get their cases from a child and read them as read-only file mappings, so that the restatement's
# arrays never pass through the heap of the process that runs the GPU suite (LABBOOK.md).

BINS = (0, 1, 64, 256)
# kind of field -> (shift, lo, hi) of the calls
FIELDS = {"constant": (4, 3.0, 3.25), "integers": (8, 0.0, 65535.0), "noise": (14, -500.0, 750.5), "ties": (-3, -1.0e6, 2.0e6),
          "edges": (14, -1024.0, 1024.0), "ramp": (10, 0.125, 9.5)}
CASES = (("one", "constant"), ("one", "noise"), ("voronoi", "integers"), ("voronoi", "ramp"), ("random", "noise"), ("spare", "ties"),
         ("outside", "noise"), ("seams", "edges"))


def case_labels(dims, layout):
    """(labels [d, h, w] int32, n_labels)"""
    w, h, d = dims
    if layout == "seams":       # bodies that end on the seams of the 64 x 4 x 32 tiles, and a change of label on a tile's last plane
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        lab = 1 + ((x // 64) + (y // 4) + (z // 32)) % 3
        lab = np.where(z % 32 == 31, 4 + (x + y) % 2, lab)
        return lab.astype(np.int32), 5
    from test_gpu_label_motion import label_volume
    return label_volume(dims, layout)


def case_field(dims, kind):
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    shape = (d, h, w)
    shift, lo, hi = FIELDS[kind]
    if kind == "constant":
        return np.full(shape, 3.25, F32)                                  # s == hi: the last bin
    if kind == "integers":
        return rng.integers(0, 65536, shape).astype(F32)
    if kind == "ramp":
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        return (F32(0.03125) * x.astype(F32) + F32(0.0625) * y.astype(F32) + F32(0.09375) * z.astype(F32)).astype(F32)
    if kind == "ties":                                                    # (k + 0.5) * 8, exact: rint meets a tie at every voxel
        k = rng.integers(-2 ** 20, 2 ** 20, shape)
        f = ((k + 0.5) * 8.0).astype(F32)
        assert np.array_equal(f.astype(np.float64) / 8.0, k + 0.5)
        return f
    one = F32(1024.0)
    specials = np.array([1e-40, -1e-40, 1.4e-45, 0.0, -0.0, np.nextafter(one, F32(0)), -np.nextafter(one, F32(0)), 1024.0, -1024.0,
                         np.nextafter(one, F32(np.inf)), -np.nextafter(one, F32(np.inf)), np.inf, -np.inf, 0.5 / 16384, -0.5 / 16384,
                         1.5 / 16384, -1.5 / 16384, 2.5 / 16384, 750.5, -500.0, np.nextafter(F32(750.5), F32(np.inf)), 3e38, -3e38], F32)
    if kind == "edges":
        return rng.choice(specials, size=shape).astype(F32)
    assert kind == "noise"
    f = rng.uniform(-1023.0, 1023.0, shape).astype(F32)
    pick = rng.random(shape)
    k = rng.integers(-2 ** 23, 2 ** 23, shape)
    ties = ((k + 0.5) / 16384.0).astype(F32)
    f[pick < 0.10] = ties[pick < 0.10]
    m = (pick >= 0.10) & (pick < 0.20)
    f[m] = rng.choice(specials, size=int(m.sum()))
    f[(pick >= 0.20) & (pick < 0.24)] = np.nan                           # holes
    f[: max(1, d // 3), : max(1, h // 2), : max(1, w // 3)][pick[: max(1, d // 3), : max(1, h // 2), : max(1, w // 3)] > 0.5] = np.nan
    f[d // 2:d // 2 + 2, :, w // 4:w // 2] = np.nan                      # a block
    return f


def case_table(dims, layout, kind):
    """({labels, field, label_box, field_box, rows_B, counts_B ...}, settings and info): the containers are three columns, two rows and a
    plane larger than the box; the float padding is NaN and the label padding carries a valid label"""
    dims = tuple(dims)
    labels, n_labels = case_labels(dims, layout)
    field = case_field(dims, kind)
    shift, lo, hi = FIELDS[kind]
    d, h, w = labels.shape
    label_box = np.full((d + 1, h + 2, w + 3), 1, np.int32)
    label_box[:d, :h, :w] = labels
    field_box = np.full((d + 1, h + 2, w + 3), np.nan, F32)
    field_box[:d, :h, :w] = field
    arrays = dict(labels=labels, field=field, label_box=label_box, field_box=field_box)
    info = None
    for bins in BINS:
        rows, counts, info = label_field_sums(field, labels, n_labels, shift, lo, hi, bins)
        arrays[f"rows_{bins}"] = rows
        if bins:
            arrays[f"counts_{bins}"] = counts
    return arrays, dict(info=info, n_labels=n_labels, shift=shift, lo=lo, hi=hi)


def in_child(jobs, directory):
    """jobs: a list of argument lists of case_table.  A child interpreter computes them all and leaves every array as a .npy file under
    `directory`; returns a list of (dict of read-only file mappings, settings dict) in their order."""
    import json
    import os
    import subprocess
    import sys
    with open(os.path.join(directory, "jobs.json"), "w") as f:
        json.dump(jobs, f)
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, os.path.join(here, "label_field_ref.py"), directory], check=True, cwd=here, timeout=600)
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
