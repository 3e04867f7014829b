#!/usr/bin/env python3
"""Time of the overlap of two label volumes through a displacement (f3d_label_overlap) at --size^3, --reps calls per row between HIP
events round the whole blocking call (the clearing of the table, the kernel, the compaction, the copies down, the waits and the
host's sort of the rows included) after --warmup calls:
    one            one label everywhere in both volumes, no displacement: one run per lane and tile, one key
    cells          Voronoi cells of about --cell voxels across (the volume of tools/contacts_bench.py) against themselves, no
                   displacement: thousands of keys, every one on the diagonal
    cells_smooth   the same cells through a smooth displacement of a few voxels: the gather leaves the lane's own column, and every
                   body overlaps its neighbours
    random         a random label out of 2^10 at every voxel of both volumes, no displacement: nearly every voxel closes a run and
                   every tile overflows its LDS table.  The worst case, which only has to be correct
In the same invocation, as the yardstick on the same labels of A: f3d_label_motion_sums without a weight (16 B per voxel against the
20 B of A, u, v, w and B).  Every case is checked: the classes add up to the voxels, the rows to lost_body + overlap, and on the
identity cases the diagonal equals numpy's counts.
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, and compares bench.solver_kernel_stamp() of both: the solve did not move
    --skip-random        leaves the worst case out
Prints one JSON line.
    python tools/overlap_bench.py [--size 512] [--cell 30] [--reps 5] [--warmup 1] [--table PATH] [--parent-libdir DIR]"""
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


# a smooth displacement of up to about three voxels: separable waves, built plane by plane
grid = np.arange(S, dtype=np.float32)
waves = [np.float32(3.0) * np.sin(np.float32(2 * np.pi / 97.0) * grid + np.float32(p)) for p in (0.3, 1.1, 2.3)]
smooth = [(waves[0][None, :, None] * np.cos(np.float32(0.01) * grid)[:, None, None] + np.zeros((1, 1, S), np.float32)),
          (waves[1][None, None, :] + np.zeros((S, S, 1), np.float32)) * np.float32(0.7),
          (waves[2][None, :, None] + np.zeros((S, 1, S), np.float32)) * np.float32(0.5)]
overlap_fn = f3d._overlap_entry()
label_sums_fn, _ = f3d._label_motion_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
disp = [box.new(np.ascontiguousarray(c, dtype=np.float32)) for c in smooth]
del smooth
labels_a, labels_b = box.alloc(), box.alloc()
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


result = {"size": S, "reps": a.reps}
rows = []


def record(name, need, call, extra=None):
    mean, best = timed(name, call)
    result[name] = {"ms": round(mean, 4), "min_ms": round(best, 4), "compulsory_B_per_voxel": need,
                    "TBps_compulsory": round(need * vox / (mean * 1e-3) / 1e12, 3)}
    if extra:
        result[name].update(extra)
    rows.append((name, mean, best, need, result[name]["TBps_compulsory"]))


def complete(n_a, n_b, d, first=None):
    """the first call with room enough, as OpticalFlowE::ComputeOverlap finds it: (rows, info, capacity)"""
    capacity = first or min(8 * (n_a + n_b), 1 << 20)
    while True:
        out, info = (f3d.Overlap * capacity)(), f3d.OverlapInfo()
        f3d.check(overlap_fn(labels_a, n_a, labels_b, n_b, *d, S, S, S, capacity, out, C.byref(info)), "f3d_label_overlap")
        if info.complete or capacity >= (1 << 24):
            return out, info, capacity
        capacity = min(2 * capacity, 1 << 24)


cases = [("one", lambda: (np.ones((S, S, S), np.int32), 1), [0, 0, 0]), ("cells", lambda: cells(S, a.cell), [0, 0, 0]), ("cells_smooth", None, disp)]
if not a.skip_random:
    cases.append(("random", lambda: (rng.integers(1, (1 << 10) + 1, (S, S, S), dtype=np.int32), 1 << 10), [0, 0, 0]))
n = 0
voxels = None
for name, make, d in cases:
    if make is not None:
        labels, n = make()
        box.upload(labels_a, labels.view(np.float32))
        if name == "random":
            labels = rng.integers(1, (1 << 10) + 1, (S, S, S), dtype=np.int32)
        box.upload(labels_b, labels.view(np.float32))
        voxels = np.bincount(labels.ravel(), minlength=n + 1)[1:] if name != "random" else None
        del labels
    out, info, capacity = complete(n, n, d, (1 << 21) if name == "random" else None)   # 2^20 possible pairs: no climbing up to them
    table = np.frombuffer(out, f3d._OVERLAP_DTYPE, count=int(info.n_pairs) if info.complete else 0)
    classes = info.foreign_a + info.lost_background + info.lost_body + info.foreign_b + info.background + info.overlap
    good = classes == vox and (not info.complete or int(table["n"].sum()) == info.lost_body + info.overlap)
    if name in ("one", "cells"):
        good = good and info.complete and np.array_equal(table["a"], table["b"]) and np.array_equal(table["n"], voxels[table["a"] - 1].astype(np.uint64))
    if not good:
        raise SystemExit(f"{name}: {info.as_dict()} does not add up")
    record(f"overlap_{name}", 20 if d[0] else 8,
           lambda: overlap_fn(labels_a, n, labels_b, n, *d, S, S, S, capacity, out, C.byref(info)),
           {"labels": n, "capacity": capacity, "pairs": int(info.n_pairs), "complete": int(info.complete), "lost_body": int(info.lost_body),
            "copied_down_MB": round(int(info.n_pairs) * 64 / 1e6, 2)})
    motion = (f3d.MotionSums * n)()
    record(f"label_sums_{name}", 16, lambda: label_sums_fn(*disp, labels_a, n, 0, 0.0, S, S, S, motion, None))
    result[f"overlap_{name}_over_label_sums"] = round(result[f"overlap_{name}"]["ms"] / result[f"label_sums_{name}"]["ms"], 3)
    del motion
    print(json.dumps({k: v for k, v in result.items() if k.endswith(name) or f"_{name}_" in k}), flush=True)
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
        f.write(f"overlap of two label volumes at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls\n")
        f.write(f"{'call':<28}{'mean ms':>10}{'min ms':>10}{'B/voxel':>9}{'TB/s':>8}\n")
        for name, mean, best, need, rate in rows:
            f.write(f"{name:<28}{mean:>10.4f}{best:>10.4f}{need:>9}{rate:>8.3f}\n")
        for name, _, _ in cases:
            r = result[f"overlap_{name}"]
            f.write(f"{name}: {r['labels']} labels, {r['pairs']} pairs in room for {r['capacity']}, {r['copied_down_MB']} MB copied down, "
                    f"{r['lost_body']} body voxels lost, overlap / f3d_label_motion_sums {result[f'overlap_{name}_over_label_sums']}\n")
        if "bench" in result:
            stamp = result["solver_kernel_stamp"]
            f.write(f"solver_kernel_stamp this {stamp['this']} parent {stamp['parent']}\n")
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        f"   (--gpus 1 --steps 3 --warmup 1, {S}^3)\n")
print(json.dumps(result), flush=True)
