#!/usr/bin/env python3
"""Time of the polar decomposition kernel (f3d_polar_decomposition, k_polar) at --size^3: principal_bench.py's smooth random
displacement, then --reps launches per configuration between HIP events after --warmup launches: each of the seven selections of the
groups angle, vector, stretch, without and with the statistics (the second, one-workgroup launch and the read-back included), and,
in the same run as the yardstick, f3d_principal_strain storing all ten of its fields.  Rates are over the compulsory bytes (12 B read
+ 4 B per stored field per voxel); `of_yardstick` is the time over the yardstick's.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/polar_bench.py` for the kernel times themselves.  Prints one JSON line.
    python tools/polar_bench.py [--size 512] [--reps 20] [--warmup 3]"""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3
rng = np.random.default_rng(1)
z = np.arange(S, dtype=np.float32)
# smooth: a few voxels of displacement varying over tens of voxels, plus a little noise
base = [(np.sin(z / 17.0 + k)[:, None, None] * np.cos(z / 23.0 - k)[None, :, None] * np.sin(z / 29.0 + 2 * k)[None, None, :]
         * np.float32(3)).astype(np.float32) for k in range(3)]
comps = [(b + rng.standard_normal(size=(S, S, S), dtype=np.float32) * np.float32(0.05)).astype(np.float32) for b in base]
polar = f3d._polar_entry()
principal = f3d._principal_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
del comps, base
outs = [box.alloc() for _ in range(10)]
box.set_current()
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))

R_GROUPS = (1, 2, 2, 2, 4, 4, 4)
P_GROUPS = (1, 1, 1, 2, 4, 4, 4, 8, 8, 8)
SELECTIONS = {1: "angle", 2: "vector", 3: "angle_vector", 4: "stretch", 5: "angle_stretch", 6: "vector_stretch", 7: "all7"}
configs = [("principal_all10", principal, P_GROUPS, 15, None)]
for mask, name in SELECTIONS.items():
    configs += [(name, polar, R_GROUPS, mask, None), (name + "_stats", polar, R_GROUPS, mask, f3d.PolarStats())]
result = {"size": S, "reps": a.reps}
for name, fn, groups, mask, stats in configs:
    stored = sum(1 for g in groups if mask & g)
    arr = (f3d._dp * len(groups))(*[p if mask & g else 0 for p, g in zip(outs, groups)])
    for _ in range(a.warmup):
        f3d.check(fn(*ins, arr, mask, S, S, S, stats), name)
    f3d.sync()
    f3d.check(hip.f3d_event_record(ev[0]))
    for _ in range(a.reps):
        f3d.check(fn(*ins, arr, mask, S, S, S, stats), name)
    f3d.check(hip.f3d_event_record(ev[1]))
    f3d.check(hip.f3d_event_sync(ev[1]))
    ms = C.c_float()
    f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
    per = ms.value / a.reps
    nbytes = (12 + 4 * stored) * vox
    result[name] = {"ms": round(per, 4), "bytes_per_voxel": 12 + 4 * stored, "TBps": round(nbytes / (per * 1e-3) / 1e12, 3),
                    "of_yardstick": round(per / result["principal_all10"]["ms"], 3) if name != "principal_all10" else 1.0}
    if stats is not None:
        result[name].update(stats.as_dict())
for e in ev:
    hip.f3d_event_destroy(e)
box.free()
print(json.dumps(result), flush=True)
