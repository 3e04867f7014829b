#!/usr/bin/env python3
"""Time of the principal strain kernel (f3d_principal_strain, k_principal_strain) at --size^3: strain_bench.py's smooth random
displacement, then --reps launches per configuration between HIP events after --warmup launches: the three values alone, values +
maximum shear (both without the eigenvector matrix), all ten fields, all ten with the statistics (the second, one-workgroup launch
and the read-back included), all ten on a field with --lost (default 10 %) of its voxels lost (NaN), and, in the same call as the
yardstick, f3d_flow_strain storing all eight of its fields.  Rates are over the compulsory bytes (12 B read + 4 B per stored field
per voxel); the launch is expected at the vector-issue bound, not at HBM's, so the time per voxel of one CU (256 of them share the
volume) is given as well.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/principal_bench.py` for the kernel times
themselves.  Prints one JSON line.
    python tools/principal_bench.py [--size 512] [--reps 20] [--warmup 3] [--lost 0.1]"""
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
ap.add_argument("--lost", type=float, default=0.1)
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
principal = f3d._principal_entry()
strain = f3d._strain_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
lost = rng.random(size=(S, S, S), dtype=np.float32) < a.lost
for c in comps:
    c[lost] = np.nan
ins_lost = [box.new(c) for c in comps]
del comps, base
outs = [box.alloc() for _ in range(10)]
box.set_current()
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))

P_GROUPS = (1, 1, 1, 2, 4, 4, 4, 8, 8, 8)
S_GROUPS = (1, 2, 2, 2, 2, 2, 2, 4)
configs = [("val", principal, P_GROUPS, 1, ins, False), ("val_shear", principal, P_GROUPS, 3, ins, False),
           ("all10", principal, P_GROUPS, 15, ins, False), ("all10_stats", principal, P_GROUPS, 15, ins, True),
           ("all10_lost", principal, P_GROUPS, 15, ins_lost, False), ("flow_strain_all8", strain, S_GROUPS, 7, ins, False)]
result = {"size": S, "reps": a.reps, "lost_fraction": a.lost}
for name, fn, groups, mask, src, want_stats in configs:
    stored = sum(1 for g in groups if mask & g)
    arr = (f3d._dp * len(groups))(*[p if mask & g else 0 for p, g in zip(outs, groups)])
    stats = f3d.PrincipalStats() if want_stats else None
    for _ in range(a.warmup):
        f3d.check(fn(*src, arr, mask, S, S, S, stats), name)
    f3d.sync()
    f3d.check(hip.f3d_event_record(ev[0]))
    for _ in range(a.reps):
        f3d.check(fn(*src, arr, mask, S, S, S, stats), name)
    f3d.check(hip.f3d_event_record(ev[1]))
    f3d.check(hip.f3d_event_sync(ev[1]))
    ms = C.c_float()
    f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
    per = ms.value / a.reps
    nbytes = (12 + 4 * stored) * vox
    tbps = nbytes / (per * 1e-3) / 1e12
    result[name] = {"ms": round(per, 4), "bytes_per_voxel": 12 + 4 * stored, "TBps": round(tbps, 3),
                    "of_achievable_6_3": round(tbps / 6.3, 3), "ns_per_voxel_of_one_cu": round(per * 1e6 / vox * 256, 3)}
    if want_stats:
        result[name].update(stats.as_dict())
for e in ev:
    hip.f3d_event_destroy(e)
box.free()
print(json.dumps(result), flush=True)
