#!/usr/bin/env python3
"""Time of the local correlation (f3d_local_correlation, k_local_correlation) on a real pair: the synthetic pair of --size^3 is
solved once with the default parameters, frame 1 is carried onto frame 0's grid through the flow, then --reps launches per
configuration between HIP events after --warmup launches: radius 1 .. 4, each storing zncc only and both fields, with and without the
statistics (the second, one-workgroup launch and the read-back included).  In the same call, as yardsticks, f3d_carry_field (linear)
of frame 1 through the flow and f3d_flow_strain of the flow with all eight outputs.  Per configuration the share of the solve, the
bytes the call must move (8 B read + 4 B per stored field per voxel) as a rate, and the redundancy of the kernel's 32 x 8 x 32 tile
(rows the x sums are formed for, planes marched, points loaded -- each over the voxels stored).
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Run it under `rocprofv3 --kernel-trace --stats -- python tools/correlation_bench.py` for the kernel times themselves.  Prints one JSON
line.
    python tools/correlation_bench.py [--size 512] [--reps 10] [--warmup 2] [--parent-libdir DIR]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

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
TX, TY, TZ = 32, 8, 32   # k_local_correlation's tile of a plane and its run of planes


def redundancy(r):
    """what the tile does beyond one x sum, one plane and one load per voxel, on a volume of whole tiles"""
    return {"x_sum_rows": round((TY + 2 * r) / TY, 3), "planes": round((TZ + 2 * r) / TZ, 3),
            "points_loaded": round((TX + 2 * r) * (TY + 2 * r) * (TZ + 2 * r) / (TX * TY * TZ), 3)}


f0, f1 = f3d.synth_pair(S, S, S)
flow = f3d.OpticalFlow()
flow.initialize(S, S, S)
flow.upload(f0, f1)
solve_s = flow.compute_resident(silent=True)
comps = flow.download()
flow.destroy()

correlation, carry, strain = f3d._correlation_entry(), f3d._carry_entry(), f3d._strain_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
frame_0, frame_1 = box.new(f0), box.new(f1)
del f0, f1, comps
warped = box.alloc()
outs = [box.alloc() for _ in range(8)]
box.set_current()
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))


def timed(name, call):
    for _ in range(a.warmup):
        f3d.check(call(), name)
    f3d.sync()
    total = 0.0
    for _ in range(a.reps):
        f3d.check(hip.f3d_event_record(ev[0]))
        f3d.check(call(), name)
        f3d.check(hip.f3d_event_record(ev[1]))
        f3d.check(hip.f3d_event_sync(ev[1]))
        ms = C.c_float()
        f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
        total += ms.value
    return total / a.reps


result = {"size": S, "reps": a.reps, "solve_s": round(solve_s, 4)}
ms = timed("f3d_carry_field", lambda: carry(frame_1, *ins, warped, S, S, S, 1, None))
result["carry_linear"] = {"ms": round(ms, 4), "TBps_at_20_B": round(20 * vox / (ms * 1e-3) / 1e12, 3)}
ms = timed("f3d_flow_strain", lambda: strain(*ins, (f3d._dp * 8)(*outs), 7, S, S, S, None))
result["strain_all_eight"] = {"ms": round(ms, 4), "TBps_at_44_B": round(44 * vox / (ms * 1e-3) / 1e12, 3)}
for r in (1, 2, 3, 4):
    for mask, fields in ((1, "zncc"), (3, "both")):
        for with_stats in (False, True):
            stats = f3d.CorrelationStats() if with_stats else None
            name = f"r{r}_{fields}" + ("_stats" if with_stats else "")
            ms = timed(name, lambda: correlation(frame_0, warped, (f3d._dp * 2)(outs[0], outs[1]), mask, r, 0.8, S, S, S, stats))
            need = 8 + 4 * bin(mask).count("1")
            result[name] = {"ms": round(ms, 4), "of_a_solve": round(ms * 1e-3 / solve_s, 5), "compulsory_B_per_voxel": need,
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
