#!/usr/bin/env python3
"""The time of one f3d_block_match (k_block_match) at --size^3 on a random texture (no window is flat, so every node
searches every candidate that is inside the volume): HIP events round the blocking entry, five calls after one warm-up, for the
defaults of the package (step 16, window 8, search 8) and for coarser grids, smaller windows and wider searches (CONFIGS; window +
search may not exceed 16, so the widest search, 15, goes with a window of 1).  Beside it, in the same process on the same build, the
seconds of one solve of the benchmark's synthetic pair of that size with the default parameters (what bench.py times), so that the
cost of the guess stands next to the cost of the solve it prepares.
    --table PATH   writes the text table
Prints one JSON line.
    python tools/block_match_bench.py [--size 512] [--no-solve]"""
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
# window + search <= 16: the defaults, a coarser grid, smaller windows, and the widest search (window 1)
CONFIGS = [dict(step=16, window=8, search=8), dict(step=32, window=8, search=8), dict(step=16, window=4, search=8),
           dict(step=16, window=4, search=12), dict(step=32, window=1, search=15), dict(step=16, window=3, search=4)]

rng = np.random.default_rng(29)
frame0 = rng.integers(0, 256, size=(K, K, K), dtype=np.uint8).astype(np.float32)
frame1 = np.roll(frame0, (2, -3, 5), axis=(0, 1, 2))
hip = f3d.hip()
fn = f3d._block_match_entry()
box = f3d.Containers(K, K, K)
ptrs = [box.new(frame0), box.new(frame1)]
del frame0, frame1
box.set_current()
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))
rows = []
for cfg in CONFIGS:
    grid = f3d.block_match_grid((K, K, K), **cfg)
    nodes = grid.nx * grid.ny * grid.nz
    records, info = np.zeros((nodes, f3d.BLOCK_MATCH_RECORD_WORDS), np.int32), f3d.BlockMatchInfo()
    times = []
    for i in range(6):
        f3d.check(hip.f3d_event_record(ev[0]))
        f3d.check(fn(*ptrs, 0.0, 255.0, 256, K, K, K, C.byref(grid), None, records.ctypes.data, C.byref(info)), "f3d_block_match")
        f3d.check(hip.f3d_event_record(ev[1]))
        f3d.check(hip.f3d_event_sync(ev[1]))
        ms = C.c_float()
        f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
        if i:
            times.append(ms.value)
    products = info.evaluated * (2 * cfg["window"] + 1) ** 3
    found = int(((records[:, 0] == 5) & (records[:, 1] == -3) & (records[:, 2] == 2)).sum())
    rows.append(dict(cfg, nodes=nodes, evaluated=int(info.evaluated), outside=int(info.outside), window_products=int(products),
                     ms=[round(t, 3) for t in times], mean_ms=round(sum(times) / len(times), 3),
                     tera_products_per_s=round(products / (sum(times) / len(times) * 1e-3) / 1e12, 3), nodes_at_the_true_shift=found))
for e in ev:
    hip.f3d_event_destroy(e)
box.free()
result = {"size": K, "k_block_match": rows}
if not a.no_solve:
    f0, f1 = f3d.synth_pair(K, K, K)
    flow = f3d.OpticalFlow()
    flow.initialize(K, K, K)
    flow.upload(f0, f1)
    del f0, f1
    flow.compute_resident(silent=True)
    result["solve_s"] = [round(flow.compute_resident(silent=True), 4) for _ in range(2)]
    flow.destroy()
lines = ["f3d_block_match at %d^3 (random texture, 256 codes), five calls after a warm-up, HIP events round the blocking entry" % K,
         "step window search    nodes    candidates  window products    mean ms   Tprod/s (by the mean)"]
for r in rows:
    lines.append("%4d %6d %6d %8d %13d %16d %10.3f %9.3f" % (r["step"], r["window"], r["search"], r["nodes"], r["evaluated"],
                                                             r["window_products"], r["mean_ms"], r["tera_products_per_s"]))
if "solve_s" in result:
    lines.append("one solve of the synthetic pair of that size, default parameters: %s s" % ", ".join("%.3f" % s for s in result["solve_s"]))
if a.table:
    with open(a.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print("\n".join(lines), file=sys.stderr)
print(json.dumps(result))
