#!/usr/bin/env python3
"""Time of the strain window (f3d_window_strain, k_window_strain) at --size^3 on the smooth random displacement of
tools/strain_bench.py: --reps launches per configuration, each between HIP events, after --warmup launches: radius 1, 2, 3, storing
vol + e + eq (eight fields) and all seventeen, with and without the statistics (the second, one-workgroup launch and the read-back
included).  In the same call, as yardsticks, f3d_flow_strain with all eight outputs and f3d_local_correlation (both fields) at the
same radii on two components of the displacement.  Per configuration the ratio to both yardsticks, the bytes the call must move
(12 B read + 4 B per stored field per voxel) as a rate, and the redundancy of the kernel's 32 x 8 x 32 tile.
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move; the mean solve time of this build then
                         gives every configuration's share of a solve
Run it under `rocprofv3 --kernel-trace --stats -- python tools/window_strain_bench.py` for the kernel times themselves.  Prints one
JSON line.
    python tools/window_strain_bench.py [--size 512] [--reps 10] [--warmup 2] [--parent-libdir DIR]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-libdir")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3
TX, TY, TZ = 32, 8, 32   # k_window_strain's tile of a plane and its run of planes
GROUP_OF = (1, 2, 2, 2, 2, 2, 2, 4) + (8,) * 9


def redundancy(r):
    """what the tile does beyond one x sum, one plane and one load per voxel, on a volume of whole tiles"""
    return {"x_sum_rows": round((TY + 2 * r) / TY, 3), "planes": round((TZ + 2 * r) / TZ, 3),
            "points_loaded": round((TX + 2 * r) * (TY + 2 * r) * (TZ + 2 * r) / (TX * TY * TZ), 3)}


rng = np.random.default_rng(1)
z = np.arange(S, dtype=np.float32)
# smooth: a few voxels of displacement varying over tens of voxels, plus a little noise
base = [(np.sin(z / 17.0 + k)[:, None, None] * np.cos(z / 23.0 - k)[None, :, None] * np.sin(z / 29.0 + 2 * k)[None, None, :]
         * np.float32(3)).astype(np.float32) for k in range(3)]
comps = [(b + rng.standard_normal(size=(S, S, S), dtype=np.float32) * np.float32(0.05)).astype(np.float32) for b in base]
window, strain, correlation = f3d._window_strain_entry(), f3d._strain_entry(), f3d._correlation_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
del comps, base
outs = [box.alloc() for _ in GROUP_OF]
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
    return sum(times) / len(times), min(times), max(times)


result = {"size": S, "reps": a.reps}
strain_ms, lo, hi = timed("f3d_flow_strain", lambda: strain(*ins, (f3d._dp * 8)(*outs[:8]), 7, S, S, S, None))
result["strain_all_eight"] = {"ms": round(strain_ms, 4), "min": round(lo, 4), "max": round(hi, 4),
                              "TBps_at_44_B": round(44 * vox / (strain_ms * 1e-3) / 1e12, 3)}
for r in (1, 2, 3):
    corr_ms, lo, hi = timed(f"correlation_r{r}", lambda: correlation(ins[0], ins[1], (f3d._dp * 2)(outs[0], outs[1]), 3, r, 0.8, S, S, S,
                                                                   None))
    result[f"correlation_r{r}_both"] = {"ms": round(corr_ms, 4), "min": round(lo, 4), "max": round(hi, 4)}
    min_count = max(4, (2 * r + 1) ** 3 // 4)
    for mask, fields in ((7, "strain8"), (15, "all17")):
        arr = (f3d._dp * 17)(*[p if mask & g else 0 for p, g in zip(outs, GROUP_OF)])
        stored = sum(1 for g in GROUP_OF if mask & g)
        for with_stats in (False, True):
            stats = f3d.WindowStrainStats() if with_stats else None
            name = f"r{r}_{fields}" + ("_stats" if with_stats else "")
            ms, lo, hi = timed(name, lambda: window(*ins, arr, mask, r, min_count, S, S, S, stats))
            need = 12 + 4 * stored
            result[name] = {"ms": round(ms, 4), "min": round(lo, 4), "max": round(hi, 4), "x_flow_strain": round(ms / strain_ms, 2),
                            "x_local_correlation": round(ms / corr_ms, 2), "compulsory_B_per_voxel": need,
                            "TBps_compulsory": round(need * vox / (ms * 1e-3) / 1e12, 3), "redundancy": redundancy(r)}
            if with_stats:
                result[name].update(stats.as_dict())
for e in ev:
    hip.f3d_event_destroy(e)
box.free()

if a.parent_libdir:
    # the solve against the parent's libraries, alternating, every run a fresh process
    runs = {"this": [], "parent": []}
    for which in ("this", "parent", "this", "parent"):
        env = dict(os.environ)
        if which == "parent":
            env["F3D_LIBDIR"] = os.path.abspath(a.parent_libdir)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(S)],
                           env=env, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not line:
            raise SystemExit(f"bench.py ({which}) failed: {p.stdout[-500:]} {p.stderr[-1500:]}")
        runs[which].append(json.loads(line[-1]))
    result["bench"] = runs
print(json.dumps(result), flush=True)
