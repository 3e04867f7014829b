#!/usr/bin/env python3
"""Time of the per-label statistics of a field (f3d_label_field_sums) at --size^3, --reps calls per row between HIP events round the
whole blocking call (the clearing of the rows and counts, the kernel, the copy down, the wait and the conversion of the rows included)
after --warmup calls, each volume with bins = 0 and with bins = 64:
    one            one label everywhere, a constant field: one run per lane and tile, one (label, bin) pair
    cells_smooth   Voronoi cells of about --cell voxels across (the volume of tools/contacts_bench.py) with a smooth field: thousands of
                   labels, long runs of equal bins along z
    cells_noise    the same cells with Gaussian noise: nearly every voxel closes its run of equal (label, bin)
    random         a random label out of 2^10 at every voxel with the noise: nearly every voxel closes both runs and every tile overflows
                   both LDS tables.  The worst case, which only has to be correct
In the same invocation, as the yardstick on the same labels: f3d_label_motion_sums without a weight (16 B per voxel against the 8 B of
the field and the labels).  Every case is checked: the classes add up to the voxels, n per label is numpy's count, and with bins
below + above + the counts of a label add up to its n.  f3d_paint_labels is timed on the cells.
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, and compares bench.solver_kernel_stamp() of both: the solve did not move
    --skip-random        leaves the worst case out
Prints one JSON line.  The other histogram route (global adds of the merged runs alone) is the same source built with
-DF3D_LABEL_FIELD_DIRECT; run this tool with F3D_LIBDIR on such a build to time it.
    python tools/label_field_bench.py [--size 512] [--cell 30] [--reps 5] [--warmup 1] [--table PATH] [--parent-libdir DIR]"""
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
ap.add_argument("--cell", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--table")
ap.add_argument("--parent-libdir")
ap.add_argument("--skip-random", action="store_true")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3
rng = np.random.default_rng(0)
BINS = 64


def cells(size, across):
    """labels 1 .. g^3 of the nearest of g^3 seeds jittered on a grid of pitch `across`, at half the size and doubled along each axis"""
    half, pitch = (size + 1) // 2, max(2.0, across / 2.0)
    g = int(np.ceil(half / pitch))
    seeds = (np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1) + rng.random((g, g, g, 3))) * pitch      # [gz, gy, gx, zyx]
    out = np.empty((half, half, half), np.int32)
    y, x = np.meshgrid(np.arange(half, dtype=np.float32), np.arange(half, dtype=np.float32), indexing="ij")
    cy, cx = (y / pitch).astype(np.int64), (x / pitch).astype(np.int64)
    for z in range(half):
        cz = int(z / pitch)
        best = np.full((half, half), np.inf, np.float32)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    iz, iy, ix = min(max(cz + dz, 0), g - 1), np.clip(cy + dy, 0, g - 1), np.clip(cx + dx, 0, g - 1)
                    s = seeds[iz, iy, ix]
                    dist = ((z - s[..., 0]) ** 2 + (y - s[..., 1]) ** 2 + (x - s[..., 2]) ** 2).astype(np.float32)
                    closer = dist < best
                    best[closer] = dist[closer]
                    out[z][closer] = (1 + (iz * g + iy) * g + ix)[closer]
    return np.repeat(np.repeat(np.repeat(out, 2, 0), 2, 1), 2, 2)[:size, :size, :size].copy(), g ** 3


# a smooth strain-like field: separable waves of a few per cent
grid = np.arange(S, dtype=np.float32)
wave = [np.float32(0.01) * np.sin(np.float32(2 * np.pi / p) * grid + np.float32(q)) for p, q in ((97.0, 0.3), (131.0, 1.1), (61.0, 2.3))]
smooth = np.ascontiguousarray(wave[0][None, None, :] + wave[1][None, :, None] + wave[2][:, None, None], dtype=np.float32)
field_fn, paint_fn = f3d._label_field_entry(), f3d._paint_entry()
label_sums_fn, _ = f3d._label_motion_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
field, labels_c = box.alloc(), box.alloc()
others = [box.new(smooth), box.new(smooth)]        # the v and w of the yardstick, which reads three fields
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


result = {"size": S, "reps": a.reps, "libdir": os.environ.get("F3D_LIBDIR", "")}
rows = []


def record(name, need, call, extra=None):
    mean, best = timed(name, call)
    result[name] = {"ms": round(mean, 4), "min_ms": round(best, 4), "compulsory_B_per_voxel": need,
                    "TBps_compulsory": round(need * vox / (mean * 1e-3) / 1e12, 3)}
    if extra:
        result[name].update(extra)
    rows.append((name, mean, best, need, result[name]["TBps_compulsory"]))


noise = None
cases = [("one", "constant"), ("cells_smooth", "smooth"), ("cells_noise", "noise")] + ([] if a.skip_random else [("random", "noise")])
n, labels = 0, None
for name, kind in cases:
    if name == "one":
        labels, n = np.ones((S, S, S), np.int32), 1
    elif name == "cells_smooth":
        labels, n = cells(S, a.cell)
    elif name == "random":
        labels, n = rng.integers(1, (1 << 10) + 1, (S, S, S), dtype=np.int32), 1 << 10
    if name != "cells_noise":
        box.upload(labels_c, labels.view(np.float32))
        voxels = np.bincount(labels.ravel(), minlength=n + 1)[1:].astype(np.uint64)
    if kind == "constant":
        values, lo, hi = np.full((S, S, S), 0.0125, np.float32), 0.0, 0.025
    elif kind == "smooth":
        values = smooth
    elif noise is None:
        values = noise = rng.standard_normal((S, S, S), dtype=np.float32) * np.float32(0.01)
    else:
        values = noise
    if kind != "constant":
        lo, hi = float(values.min()), float(values.max())
    box.upload(field, values)
    shift = f3d.label_field_shift(lo, hi)
    for bins in (0, BINS):
        out, info = (f3d.LabelFieldSumsRow * n)(), f3d.LabelFieldInfo()
        counts = np.zeros((n, bins), np.uint32) if bins else None
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint)) if bins else None
        call = lambda: field_fn(field, labels_c, n, shift, lo, hi, bins, S, S, S, out, cp, C.byref(info))
        f3d.check(call(), "f3d_label_field_sums")
        table = np.frombuffer(out, f3d._FIELD_SUMS_DTYPE)
        good = sum(info.as_dict().values()) == vox and info.used == vox and np.array_equal(table["n"], voxels)
        if bins:
            good = good and np.array_equal(table["below"] + table["above"] + counts.sum(axis=1, dtype=np.uint64), table["n"])
        if not good:
            raise SystemExit(f"{name} bins {bins}: {info.as_dict()} does not add up")
        record(f"field_{name}_bins{bins}", 8, call, {"labels": n, "shift": shift, "copied_down_MB": round((n * 64 + n * bins * 4) / 1e6, 2)})
    motion = (f3d.MotionSums * n)()
    record(f"label_sums_{name}", 16, lambda: label_sums_fn(field, *others, labels_c, n, 0, 0.0, S, S, S, motion, None))
    for bins in (0, BINS):
        result[f"field_{name}_bins{bins}_over_label_sums"] = round(result[f"field_{name}_bins{bins}"]["ms"] / result[f"label_sums_{name}"]["ms"], 3)
    del motion
    if name == "cells_noise":
        means = (table["iq"] / np.maximum(table["n"], 1)).astype(np.float32)
        painted = box.alloc()
        record("paint_cells", 8, lambda: paint_fn(labels_c, n, means.ctypes.data_as(f3d._fp), painted, S, S, S))
    print(json.dumps({k: v for k, v in result.items() if f"_{name}" in k}), flush=True)
for e in ev:
    hip.f3d_event_destroy(e)
box.free()

if a.parent_libdir:
    # the solve against the parent's libraries, alternating, every run a fresh process; and the machine code of the solver kernels
    import bench
    result["solver_kernel_stamp"] = {"this": bench.solver_kernel_stamp(),
                                     "parent": bench.solver_kernel_stamp(os.path.join(os.path.abspath(a.parent_libdir), "libf3d_hip.so"))}
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
        f.write(f"per-label statistics of a field at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls"
                f"{' (libraries of ' + result['libdir'] + ')' if result['libdir'] else ''}\n")
        f.write(f"{'call':<32}{'mean ms':>10}{'min ms':>10}{'B/voxel':>9}{'TB/s':>8}\n")
        for name, mean, best, need, rate in rows:
            f.write(f"{name:<32}{mean:>10.4f}{best:>10.4f}{need:>9}{rate:>8.3f}\n")
        for name, _ in cases:
            r = result[f"field_{name}_bins0"]
            f.write(f"{name}: {r['labels']} labels, shift {r['shift']}; call / f3d_label_motion_sums {result[f'field_{name}_bins0_over_label_sums']} "
                    f"(bins 0), {result[f'field_{name}_bins{BINS}_over_label_sums']} (bins {BINS})\n")
        if "bench" in result:
            stamp = result["solver_kernel_stamp"]
            f.write(f"solver_kernel_stamp this {stamp['this']} parent {stamp['parent']}\n")
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        f"   (--gpus 1 --steps 3 --warmup 1, {S}^3)\n")
print(json.dumps(result), flush=True)
