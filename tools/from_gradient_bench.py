#!/usr/bin/env python3
"""Time of the from-gradient kernels (f3d_principal_from_gradient, f3d_polar_from_gradient) at --size^3 on the smooth random
displacement of tools/strain_bench.py: its window gradient (f3d_window_strain, F3D_WSTRAIN_G alone, radius --radius) is left in nine
containers, and every selection of the groups of both entries runs on it, without and with the statistics (the second,
one-workgroup launch and the read-back included): --reps launches per configuration, each between HIP events, after --warmup
launches.  In the same call the stencil sibling (f3d_principal_strain, f3d_polar_decomposition) runs every one of the same
selections on the displacement, and the window pass itself is timed.  Per configuration mean / min / max, the ratio to the sibling
with the same selection (`x_sibling`), and the compulsory bytes (36 B read + 4 B per stored field per voxel) as a rate.
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Run it under `rocprofv3 --kernel-trace --stats -- python tools/from_gradient_bench.py` for the kernel times themselves.  Prints one
JSON line.
    python tools/from_gradient_bench.py [--size 512] [--reps 10] [--warmup 2] [--radius 2] [--parent-libdir DIR]"""
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
ap.add_argument("--radius", type=int, default=2)
ap.add_argument("--parent-libdir")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3
P_GROUPS = (1, 1, 1, 2, 4, 4, 4, 8, 8, 8)
R_GROUPS = (1, 2, 2, 2, 4, 4, 4)
P_NAMES = {1: "val", 2: "shear", 4: "dir1", 8: "dir3"}
R_NAMES = {1: "angle", 2: "vector", 4: "stretch"}

rng = np.random.default_rng(1)
z = np.arange(S, dtype=np.float32)
# smooth: a few voxels of displacement varying over tens of voxels, plus a little noise
base = [(np.sin(z / 17.0 + k)[:, None, None] * np.cos(z / 23.0 - k)[None, :, None] * np.sin(z / 29.0 + 2 * k)[None, None, :]
         * np.float32(3)).astype(np.float32) for k in range(3)]
comps = [(b + rng.standard_normal(size=(S, S, S), dtype=np.float32) * np.float32(0.05)).astype(np.float32) for b in base]
window = f3d._window_strain_entry()
entries = {"principal": (f3d._principal_from_gradient_entry(), f3d._principal_entry(), P_GROUPS, P_NAMES, f3d.PrincipalStats),
           "polar": (f3d._polar_from_gradient_entry(), f3d._polar_entry(), R_GROUPS, R_NAMES, f3d.PolarStats)}
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
del comps, base
grad = [box.alloc() for _ in range(9)]
outs = [box.alloc() for _ in range(10)]
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
    return {"ms": round(sum(times) / len(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


result = {"size": S, "reps": a.reps, "radius": a.radius}
min_count = max(4, (2 * a.radius + 1) ** 3 // 4)
g_arr = (f3d._dp * 9)(*grad)
w_arr = (f3d._dp * 17)(*([0] * 8 + grad))
result["window_grad_only"] = timed("f3d_window_strain", lambda: window(*ins, w_arr, 8, a.radius, min_count, S, S, S, None))
for kind, (from_gradient, sibling, groups, names, Stats) in entries.items():
    for mask in range(1, 1 << len(names)):
        label = "_".join(n for bit, n in names.items() if mask & bit)
        stored = sum(1 for g in groups if mask & g)
        arr = (f3d._dp * len(groups))(*[p if mask & g else 0 for p, g in zip(outs, groups)])
        for with_stats in (False, True):
            stats = Stats() if with_stats else None
            name = f"{kind}_{label}" + ("_stats" if with_stats else "")
            old = timed(name + " (stencil)", lambda: sibling(*ins, arr, mask, S, S, S, stats))
            new = timed(name, lambda: from_gradient(g_arr, arr, mask, S, S, S, stats))
            need = 36 + 4 * stored
            new.update(sibling_ms=old["ms"], x_sibling=round(new["ms"] / old["ms"], 3), compulsory_B_per_voxel=need,
                       TBps_compulsory=round(need * vox / (new["ms"] * 1e-3) / 1e12, 3))
            if with_stats:
                new.update(stats.as_dict())
            result[name] = new
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
