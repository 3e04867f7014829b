#!/usr/bin/env python3
"""Time of the displacement validation (f3d_validate_displacement) on a real flow: the synthetic pair of --size^3 is solved once with
the default parameters, then --reps calls per configuration between HIP events round the whole call after --warmup calls: step 1 and
4, MARK and REPLACE, with and without a weight volume, with and without the statistics (the fold, the read-back and the wait
included), and r alone / the displacement alone.  In the same run, as the yardstick, three f3d_median launches of diameter 3 on the
same three fields: the closest existing work, 27-element selections on the same neighbourhoods.  The compulsory traffic of a call is
12 B (16 B with a weight) read and 4 to 16 B written per voxel.
    --table PATH         also writes the numbers as a text table
Prints one JSON line.
    python tools/validate_bench.py [--size 512] [--reps 10] [--warmup 2] [--table PATH]"""
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
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--table")
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

fn = f3d._validate_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
weight = box.new(f0 * (1.0 / 255.0))     # any volume with values on both sides of the minimum
del f0, f1, comps
outs = [box.alloc() for _ in range(4)]
box.set_current()
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))


def timed(name, call):
    for _ in range(a.warmup):
        call()
    f3d.sync()
    times = []
    for _ in range(a.reps):
        f3d.check(hip.f3d_event_record(ev[0]))
        call()
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
                    "TBps_compulsory": round(need * vox / (mean * 1e-3) / 1e12, 3)}
    if extra:
        result[name].update(extra())
    rows.append((name, mean, best, need, result[name]["TBps_compulsory"]))


def medians():
    for i in range(3):
        f3d.check(hip.f3d_median(ins[i], S, S, S, 3, outs[i], None), "f3d_median")


record("median3_x3", 24, medians)
st = f3d.ValidateStats()
out4 = (C.c_uint64 * 4)(*outs)


def validate(step, mode, with_weight, with_stats, fields=3):
    f3d.check(fn(*ins, weight if with_weight else 0, 0.5, step, 0.1, 2.0, 9, mode, out4, fields, S, S, S, C.byref(st) if with_stats else None),
              "f3d_validate_displacement")


for step in (1, 4):
    for mode, mode_name in ((1, "mark"), (2, "replace")):
        for with_weight in (False, True):
            for with_stats in (False, True):
                name = f"step{step}_{mode_name}" + ("_weight" if with_weight else "") + ("_stats" if with_stats else "")
                record(name, (16 if with_weight else 12) + 16, lambda: validate(step, mode, with_weight, with_stats),
                       (lambda: st.as_dict()) if with_stats else None)
record("step1_replace_r_only", 12 + 4, lambda: validate(1, 2, False, False, 1))
record("step1_replace_d_only", 12 + 12, lambda: validate(1, 2, False, False, 2))
yard = result["median3_x3"]["ms"]
for name, *_ in rows[1:]:
    result[name]["over_median3_x3"] = round(result[name]["ms"] / yard, 3)
for e in ev:
    hip.f3d_event_destroy(e)
box.free()

if a.table:
    with open(a.table, "w") as f:
        f.write(f"displacement validation at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls; "
                f"solve {solve_s:.4f} s\n")
        f.write(f"{'call':<30}{'mean ms':>10}{'min ms':>10}{'B/voxel':>9}{'TB/s':>8}{'/ median3 x3':>14}\n")
        for name, mean, best, need, rate in rows:
            f.write(f"{name:<30}{mean:>10.4f}{best:>10.4f}{need:>9}{rate:>8.3f}{mean / yard:>14.3f}\n")
print(json.dumps(result), flush=True)
