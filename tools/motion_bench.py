#!/usr/bin/env python3
"""Time of the motion fit (f3d_motion_sums, f3d_remove_motion) on a real flow: the synthetic pair of --size^3 is solved once with the
default parameters, then --reps calls per configuration between HIP events after --warmup calls: the sums with and without a
weight volume (the fold, the read-back and the wait included: the entry always waits), the subtraction out of place and in place,
with and without the statistics.  In the same call, as yardsticks, f3d_flow_stats of the same three fields (it also reads u, v, w
once and reduces them) and f3d_carry_field (linear) of one field through the flow (a streaming pass of 16 B read and 4 B written per
voxel).  The host solve between the two device entries is timed with the wall clock.
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Prints one JSON line.
    python tools/motion_bench.py [--size 512] [--reps 10] [--warmup 2] [--table PATH] [--parent-libdir DIR]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--table")
ap.add_argument("--parent-libdir")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3

f0, f1 = f3d.synth_pair(S, S, S)
flow = f3d.OpticalFlow()
flow.initialize(S, S, S)
flow.upload(f0, f1)
solve_s = flow.compute_resident(silent=True)
comps = flow.download()
flow.destroy()

sums_fn, remove_fn = f3d._motion_entry()
carry = f3d._carry_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
weight = box.new(f0 * (1.0 / 255.0))     # any volume with values on both sides of the minimum
del f0, f1, comps
outs = [box.alloc() for _ in range(3)]
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


result = {"size": S, "reps": a.reps, "solve_s": round(solve_s, 4)}
rows = []


def record(name, need, call, extra=None):
    mean, best = timed(name, call)
    result[name] = {"ms": round(mean, 4), "min_ms": round(best, 4), "compulsory_B_per_voxel": need,
                    "TBps_compulsory": round(need * vox / (mean * 1e-3) / 1e12, 3), "of_a_solve": round(mean * 1e-3 / solve_s, 6)}
    if extra:
        result[name].update(extra())
    rows.append((name, mean, best, need, result[name]["TBps_compulsory"]))


lo, hi, total = C.c_float(), C.c_float(), C.c_double()
record("flow_stats", 12, lambda: hip.f3d_flow_stats(*ins, S, S, S, None, C.byref(lo), C.byref(hi), C.byref(total)))
record("carry_linear", 20, lambda: carry(ins[0], *ins, outs[0], S, S, S, 1, None))
sums = f3d.MotionSums()
record("sums", 12, lambda: sums_fn(*ins, 0, 0.0, S, S, S, C.byref(sums)), lambda: {"n": sums.n})
masked = f3d.MotionSums()
record("sums_weight", 16, lambda: sums_fn(*ins, weight, 0.5, S, S, S, C.byref(masked)), lambda: {"n": masked.n})
t0 = time.perf_counter()
fits = {m: f3d.solve_motion(sums, (S, S, S), m) for m in f3d.MOTION_MODELS}
result["host_solve_us_three_models"] = round((time.perf_counter() - t0) * 1e6, 1)
fit = fits["rigid"]
result["fit"] = fit.as_dict()
st = f3d.MotionResidual()
record("remove", 24, lambda: remove_fn(*ins, *outs, C.byref(fit), S, S, S, None))
record("remove_stats", 24, lambda: remove_fn(*ins, *outs, C.byref(fit), S, S, S, C.byref(st)), lambda: st.as_dict())
record("remove_in_place", 24, lambda: remove_fn(*outs, *outs, C.byref(fit), S, S, S, None))
result["sums_over_flow_stats"] = round(result["sums"]["ms"] / result["flow_stats"]["ms"], 3)
result["remove_over_carry"] = round(result["remove"]["ms"] / result["carry_linear"]["ms"], 3)
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

if a.table:
    with open(a.table, "w") as f:
        f.write(f"motion fit at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls; solve {solve_s:.4f} s\n")
        f.write(f"{'call':<18}{'mean ms':>10}{'min ms':>10}{'B/voxel':>9}{'TB/s':>8}{'of a solve':>12}\n")
        for name, mean, best, need, rate in rows:
            f.write(f"{name:<18}{mean:>10.4f}{best:>10.4f}{need:>9}{rate:>8.3f}{mean * 1e-3 / solve_s:>12.6f}\n")
        f.write(f"sums / flow_stats {result['sums_over_flow_stats']}, remove / carry_linear {result['remove_over_carry']}, "
                f"host solve of the three models {result['host_solve_us_three_models']} us\n")
        if "bench" in result:
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + "  ".join(json.dumps(r) for r in runs_) + "\n")
print(json.dumps(result), flush=True)
