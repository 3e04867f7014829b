#!/usr/bin/env python3
"""Time of the grey-value histogram (f3d_histogram) at --size^3 with 256 and 4096 bins on three inputs, --reps calls per row between HIP
events round the whole blocking entry (the clearing of the accumulator, the kernel, the copy of the counts down and the wait included)
after --warmup calls:
    noise      uniform noise over the whole range: every lane of a wave in another bin, no two adds of a wave on one word
    constant   one value everywhere: every lane of every wave in the same bin, the worst case for atomics on one word and the best for
               the merging of runs (one add per wave)
    two-phase  tests/golden/inputs_128.npz frame 0 (uint8 values) tiled to the size: what a tomography frame looks like
In the same invocation, on the same volume: f3d_value_range (the call in front of the histogram when no range is given) and, as the
yardstick, f3d_label_components at the Otsu cut of the 256-bin histogram (the call the histogram precedes).  Every histogram is
checked against numpy's bincount of the restated bin rule unless --skip-host.
    --table PATH   also writes the numbers as a text table
Prints one JSON line.
    python tools/histogram_bench.py [--size 512] [--reps 5] [--warmup 1] [--table PATH] [--skip-host]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--table")
ap.add_argument("--skip-host", action="store_true")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
rng = np.random.default_rng(0)
F32 = np.float32

histogram_fn, range_fn, components_fn = f3d._histogram_entry(), f3d._value_range_entry(), f3d._components_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
src = box.alloc()
labels_dev = box.alloc()
box.set_current()
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))


def timed(name, call):
    for _ in range(a.warmup):
        f3d.check(call(), name)
    f3d.sync()
    times = []
    for _ in range(a.reps):
        f3d.check(hip.f3d_event_record(ev[0]))
        f3d.check(call(), name)
        f3d.check(hip.f3d_event_record(ev[1]))
        f3d.check(hip.f3d_event_sync(ev[1]))
        ms = C.c_float()
        f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
        times.append(ms.value)
    return sum(times) / len(times), min(times)


def host_counts(volume, lo, hi, bins):
    """numpy's bincount of the bin rule of include/f3d.h (every value of these inputs lies in [lo, hi])"""
    scale = F32(bins) / (F32(hi) - F32(lo))
    return np.bincount(np.minimum(((volume.ravel() - F32(lo)) * scale).astype(np.int64), bins - 1), minlength=bins)


def tiled_frame():
    frame = np.load(os.path.join(ROOT, "tests", "golden", "inputs_128.npz"))["frame_0"].astype(F32)
    n = -(-S // frame.shape[0])
    return np.ascontiguousarray(np.tile(frame, (n, n, n))[:S, :S, :S])


result = {"size": S, "reps": a.reps}
rows = []
cases = [("noise", lambda: rng.random((S, S, S), dtype=F32), (0.0, 1.0)), ("constant", lambda: np.full((S, S, S), 0.5, F32), (0.0, 1.0)),
         ("two-phase", tiled_frame, (0.0, 255.0))]
for name, make, (lo, hi) in cases:
    volume = make()
    box.upload(src, volume)
    entry = {}
    low, high, found = C.c_float(), C.c_float(), f3d.RangeInfo()
    entry["value_range"] = timed("f3d_value_range", lambda: range_fn(src, 0, S, S, S, C.byref(low), C.byref(high), C.byref(found)))
    if found.finite != volume.size or low.value != volume.min() or high.value != volume.max():
        raise SystemExit(f"{name}: f3d_value_range gave [{low.value}, {high.value}], {found.as_dict()}")
    for bins in (256, 4096):
        counts, info = np.zeros(bins, np.uint64), f3d.HistogramInfo()
        pc = counts.ctypes.data_as(C.POINTER(C.c_ulonglong))
        entry[f"histogram_{bins}"] = timed("f3d_histogram", lambda: histogram_fn(src, 0, lo, hi, bins, S, S, S, pc, C.byref(info)))
        if info.used != volume.size or int(counts.sum()) != volume.size:
            raise SystemExit(f"{name}: {info.as_dict()} at {bins} bins")
        if not a.skip_host and not np.array_equal(counts, host_counts(volume, lo, hi, bins)):
            raise SystemExit(f"{name}: the counts at {bins} bins differ from numpy's")
        if bins == 256:
            chosen = f3d.Histogram(counts.copy(), lo, hi, info.as_dict()).otsu()
            cut = float(chosen.values[0]) if chosen.status == f3d.OTSU_OK else lo       # a constant volume has no cut: everything is one body
            entry["occupied_bins_256"] = int((counts != 0).sum())
    cinfo = f3d.ComponentInfo()
    entry["label_components"] = timed("f3d_label_components",
                                      lambda: components_fn(src, cut, float("inf"), 27, labels_dev, S, S, S, None, 0, C.byref(cinfo)))
    entry["cut"], entry["foreground"], entry["n_components"] = cut, int(cinfo.foreground), int(cinfo.n_components)
    for call in ("value_range", "histogram_256", "histogram_4096", "label_components"):
        mean, best = entry[call]
        entry[call] = {"ms": round(mean, 4), "min_ms": round(best, 4)}
        rows.append((f"{call} {name}", mean, best))
    for bins in (256, 4096):
        entry[f"histogram_{bins}_over_label_components"] = round(entry[f"histogram_{bins}"]["ms"] / entry["label_components"]["ms"], 3)
    entry["gb_per_s_256"] = round(volume.nbytes / entry["histogram_256"]["ms"] / 1e6, 1)
    result[name] = entry
    del volume
    print(json.dumps({name: entry}), flush=True)
for e in ev:
    hip.f3d_event_destroy(e)
box.free()

if a.table:
    with open(a.table, "w") as f:
        f.write(f"grey-value histogram at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls\n")
        f.write(f"{'call':<36}{'mean ms':>10}{'min ms':>10}\n")
        for name, mean, best in rows:
            f.write(f"{name:<36}{mean:>10.4f}{best:>10.4f}\n")
        for name, _, _ in cases:
            r = result[name]
            f.write(f"{name}: {r['occupied_bins_256']} of 256 bins occupied, {r['gb_per_s_256']} GB/s of source at 256 bins; histogram / "
                    f"f3d_label_components {r['histogram_256_over_label_components']} (256 bins), "
                    f"{r['histogram_4096_over_label_components']} (4096 bins); labelled at {r['cut']:.9g}: {r['foreground']} foreground voxels, "
                    f"{r['n_components']} components\n")
print(json.dumps(result), flush=True)
