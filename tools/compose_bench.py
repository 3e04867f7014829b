#!/usr/bin/env python3
"""Time of one trajectory step (f3d_compose_flow, k_compose_flow) on a real flow: the synthetic pair of --size^3 is solved once with
the default parameters, then the flow is composed into the trajectory --reps times, twice per repetition: from zero (positions on
the grid) and once more from there (positions displaced by about (2, -1, 0.5), the usual case of a sequence).  HIP events around
each step; run it under `rocprofv3 --kernel-trace --stats -- python tools/compose_bench.py` for the kernel time itself.
Prints one JSON line: mean milliseconds of each kind and the bytes per second at the compulsory 36 B per voxel.
    python tools/compose_bench.py [--size 512] [--reps 10]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
f0, f1 = f3d.synth_pair(S, S, S)
flow = f3d.OpticalFlow()
flow.initialize(S, S, S)
flow.upload(f0, f1)
solve_s = flow.compute_resident(silent=True)
hip = f3d.hip()
ev = [C.c_void_p() for _ in range(3)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))
times = {"from_zero": [], "displaced": []}
flow.trajectory_begin()
flow.trajectory_append()    # warm-up (first launch of the kernel)
for _ in range(a.reps):
    flow.trajectory_begin()
    f3d.check(hip.f3d_event_record(ev[0]))
    flow.trajectory_append()
    f3d.check(hip.f3d_event_record(ev[1]))
    flow.trajectory_append()
    f3d.check(hip.f3d_event_record(ev[2]))
    f3d.check(hip.f3d_event_sync(ev[2]))
    for kind, (b, e) in (("from_zero", (ev[0], ev[1])), ("displaced", (ev[1], ev[2]))):
        ms = C.c_float()
        f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), b, e))
        times[kind].append(ms.value)
*_, lost = flow.trajectory_download()
flow.trajectory_end()
flow.destroy()
for e in ev:
    hip.f3d_event_destroy(e)
vox = S ** 3
out = {"size": S, "reps": a.reps, "solve_s": round(solve_s, 4), "lost_after_two_steps": lost}
for kind, t in times.items():
    ms = sum(t) / len(t)
    out[kind + "_ms"] = round(ms, 4)
    out[kind + "_min_ms"] = round(min(t), 4)
    out[kind + "_TBps"] = round(36 * vox / (ms * 1e-3) / 1e12, 3)
print(json.dumps(out), flush=True)
