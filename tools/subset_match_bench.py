#!/usr/bin/env python3
"""The time of one f3d_subset_match (k_subset_match) at --size^3 on a random texture moved by whole voxels, every node
started from the truth +- 0.3 voxel: HIP events round the blocking entry, five calls after one warm-up, for step 16 with windows 4
and 8 and both models (CONFIGS).  Beside it, in the same process on the same build, the seconds of one solve of the benchmark's
synthetic pair of that size with the default parameters (what bench.py times).
    --table PATH   writes the text table
Prints one JSON line.
    python tools/subset_match_bench.py [--size 512] [--no-solve]"""
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
ap.add_argument("--table")
ap.add_argument("--no-solve", action="store_true")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
K = a.size
SHIFT = (5, -3, 2)
CONFIGS = [dict(step=16, window=4, model="translation"), dict(step=16, window=4, model="affine"),
           dict(step=16, window=8, model="translation"), dict(step=16, window=8, model="affine")]

rng = np.random.default_rng(30)
frame0 = rng.integers(0, 256, size=(K, K, K), dtype=np.uint8).astype(np.float32)
frame1 = np.roll(frame0, SHIFT[::-1], axis=(0, 1, 2))
hip = f3d.hip()
fn = f3d._subset_match_entry()
box = f3d.Containers(K, K, K)
ptrs = [box.new(frame0), box.new(frame1)]
del frame0, frame1
box.set_current()
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))
rows = []
for cfg in CONFIGS:
    # nodes far enough from the faces that the moved window and its taps stay inside
    margin = cfg["window"] + 1 + max(abs(s) for s in SHIFT) + 3
    count = (K - 2 * margin - 1) // cfg["step"] + 1
    grid = f3d.subset_grid((K, K, K), cfg["step"], cfg["window"], origin=(margin,) * 3, counts=(count,) * 3)
    nodes = count ** 3
    start = np.zeros((nodes, 12))
    start[:, 0::4] = np.asarray(SHIFT, np.float64) + rng.uniform(-0.3, 0.3, (nodes, 3))
    records, info = np.zeros(nodes, f3d.SUBSET_RECORD), f3d.SubsetInfo()
    times = []
    for i in range(6):
        f3d.check(hip.f3d_event_record(ev[0]))
        f3d.check(fn(*ptrs, K, K, K, C.byref(grid), f3d.SUBSET_MODELS[cfg["model"]], start.ctypes.data, 20, 1e-3, float(cfg["window"]),
                     records.ctypes.data, C.byref(info)), "f3d_subset_match")
        f3d.check(hip.f3d_event_record(ev[1]))
        f3d.check(hip.f3d_event_sync(ev[1]))
        ms = C.c_float()
        f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
        if i:
            times.append(ms.value)
    ok = records["status"] == 0
    error = np.abs(records["p"][ok][:, 0::4] - np.asarray(SHIFT, np.float64)).max() if ok.any() else float("nan")
    evaluations = int(info.iterations) * (2 * cfg["window"] + 1) ** 3
    mean = sum(times) / len(times)
    rows.append(dict(cfg, nodes=nodes, ok=int(ok.sum()), iterations=int(info.iterations), evaluations=evaluations,
                     ms=[round(t, 3) for t in times], mean_ms=round(mean, 3), giga_evaluations_per_s=round(evaluations / (mean * 1e-3) / 1e9, 3),
                     worst_error_of_ok=float(error)))
for e in ev:
    hip.f3d_event_destroy(e)
box.free()
result = {"size": K, "k_subset_match": rows}
if not a.no_solve:
    f0, f1 = f3d.synth_pair(K, K, K)
    flow = f3d.OpticalFlow()
    flow.initialize(K, K, K)
    flow.upload(f0, f1)
    del f0, f1
    flow.compute_resident(silent=True)
    result["solve_s"] = [round(flow.compute_resident(silent=True), 4) for _ in range(2)]
    flow.destroy()
lines = ["f3d_subset_match at %d^3 (random texture moved by %s, starts at the truth +- 0.3), five calls after a warm-up, HIP events round "
         "the blocking entry" % (K, SHIFT),
         "step window model          nodes       ok  iterations  interpolations    mean ms   Ginterp/s   worst |error| of ok"]
for r in rows:
    lines.append("%4d %6d %-12s %7d %8d %11d %15d %10.3f %11.3f %12.2e" % (r["step"], r["window"], r["model"], r["nodes"], r["ok"],
                                                                          r["iterations"], r["evaluations"], r["mean_ms"],
                                                                          r["giga_evaluations_per_s"], r["worst_error_of_ok"]))
if "solve_s" in result:
    lines.append("one solve of the synthetic pair of that size, default parameters: %s s" % ", ".join("%.3f" % s for s in result["solve_s"]))
if a.table:
    with open(a.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print("\n".join(lines), file=sys.stderr)
print(json.dumps(result))
