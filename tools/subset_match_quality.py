#!/usr/bin/env python3
"""Does `flow - subset` track `flow - truth`?    On the 24 x 40 x 48 pair of DESIGN.md 28, moved by (6, -4, 3), three
solves at 14 levels: cold, from the hand guess (5, -3, 2), from the block-match guess.  The subset measurement is made once and
does not see any of the flows: affine, window 3, step 6, started from a block-match table on the same nodes.  Per solve, over the
nodes the subset table accepts: the rms of |flow - truth| and the rms of |flow - subset| (the summary's `rms` with compare = the
flow at the nodes); beside them the rms of |subset - truth| and the rms error of the flow over the whole interior.
    --table PATH   writes the text table
Prints one JSON line.
    python tools/subset_match_quality.py"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import warm_start_ref as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--table")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
STEP, WINDOW, SEARCH, LEVELS = 6, 3, 7, 14

f0, f1 = ws.test_pair()
d, h, w = f0.shape
truth = np.asarray(ws.PAIR_SHIFT, np.float64)
grid = f3d.subset_grid((w, h, d), STEP, WINDOW)
origin, counts = (grid.ox, grid.oy, grid.oz), (grid.nx, grid.ny, grid.nz)
matched = f3d.block_match(f0, f1, step=STEP, window=WINDOW, search=SEARCH, origin=origin, counts=counts)
positions = [(origin[0] + i * STEP, origin[1] + j * STEP, origin[2] + k * STEP) for k in range(counts[2]) for j in range(counts[1])
             for i in range(counts[0])]
guess, _ = f3d.block_match_initial(f0, f1, step=STEP, window=WINDOW, search=SEARCH)
flow = f3d.OpticalFlow()
flow.initialize(w, h, d)
kw = dict(warp_levels_count=LEVELS)
solves = {"cold": flow.compute(f0, f1, silent=True, **kw),
          "hand guess": flow.compute(f0, f1, silent=True, initial=ws.constant_flow(f0.shape, ws.PAIR_GUESS), **kw),
          "block-match guess": flow.compute(f0, f1, silent=True, initial=guess, **kw)}
flow.destroy()
rows = []
for name, solved in solves.items():
    at_nodes = [np.array([c[z, y, x] for x, y, z in positions], np.float32) for c in solved]
    nodes = f3d.subset_match(f0, f1, grid=grid, start=(matched.u, matched.v, matched.w), compare=at_nodes)
    ok = nodes.rows["status"] == 0
    flow_error = np.stack(at_nodes, axis=1)[ok].astype(np.float64) - truth
    subset_error = nodes.records["p"][ok][:, 0::4] - truth
    rows.append(dict(solve=name, nodes=len(ok), accepted=int(ok.sum()), interior_rms=float(ws.rms_error(solved)),
                     flow_minus_truth=float(np.sqrt((flow_error ** 2).sum(axis=1).mean())), flow_minus_subset=nodes.summary["rms"],
                     subset_minus_truth=float(np.sqrt((subset_error ** 2).sum(axis=1).mean())), median_zncc=nodes.summary["median_zncc"]))
lines = ["24 x 40 x 48 pair moved by (6, -4, 3), %d levels; subsets: affine, window %d, step %d, started from block match; rms over the "
         "accepted nodes" % (LEVELS, WINDOW, STEP),
         "solve              nodes accepted  flow-truth (interior)  flow-truth (nodes)  flow-subset (nodes)  subset-truth"]
for r in rows:
    lines.append("%-18s %5d %8d %22.3f %19.3f %20.3f %13.4f" % (r["solve"], r["nodes"], r["accepted"], r["interior_rms"], r["flow_minus_truth"],
                                                                r["flow_minus_subset"], r["subset_minus_truth"]))
if a.table:
    with open(a.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print("\n".join(lines), file=sys.stderr)
print(json.dumps(rows))
