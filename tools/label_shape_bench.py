#!/usr/bin/env python3
"""Time of the shape sums of labelled bodies (f3d_label_shape_sums) at --size^3 on three label volumes, --reps calls per row between
HIP events round the whole blocking call (the clearing of the accumulator, the kernel, the copy down, the wait and the host's
reordering of the rows included) after --warmup calls:
    one      one label everywhere: one run per lane and tile, every neighbour equal
    cells    Voronoi cells of about --cell voxels across (the volume of tools/contacts_bench.py: seeds jittered on a grid, built at half
             the size and doubled), thousands of labels
    random   a random label out of 2^20 at every voxel: every voxel closes a run, every tile overflows its LDS table and the copy down is
             302 MB.  The worst case, which only has to be correct
In the same invocation, as yardsticks on the same labels: f3d_label_contacts without u, v, w (the same 4 B per voxel and the same table
idiom; not on the random volume, whose contacts exceed any capacity) and f3d_label_motion_sums without a weight (16 B per voxel).
Every case is checked against numpy's counts: the voxels of every label, and the equal-label pairs along x, y and z.
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
    --skip-random        leaves the worst case out
Prints one JSON line.
    python tools/label_shape_bench.py [--size 512] [--cell 30] [--reps 5] [--warmup 1] [--table PATH] [--parent-libdir DIR]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

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


comps = [(rng.standard_normal((S, S, S), dtype=np.float32) * np.float32(0.5) + np.float32(m)) for m in (2.0, -1.0, 0.5)]
shape_fn = f3d._label_shape_entry()
contacts_fn = f3d._contacts_entry()
label_sums_fn, _ = f3d._label_motion_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
ins = [box.new(c) for c in comps]
del comps
labels_dev = box.alloc()
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


cases = [("one", lambda: (np.ones((S, S, S), np.int32), 1)), ("cells", lambda: cells(S, a.cell))]
if not a.skip_random:
    cases.append(("random", lambda: (rng.integers(1, (1 << 20) + 1, (S, S, S), dtype=np.int32), 1 << 20)))
for name, make in cases:
    t0 = time.perf_counter()
    labels, n = make()
    built = time.perf_counter() - t0
    box.upload(labels_dev, labels.view(np.float32))
    voxels = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    equal = [int(np.count_nonzero(np.diff(labels, axis=k) == 0)) for k in (2, 1, 0)]      # along x, y, z
    del labels
    sums, info = (f3d.LabelShapeSums * n)(), f3d.LabelShapeInfo()
    f3d.check(shape_fn(labels_dev, n, S, S, S, sums, C.byref(info)), "f3d_label_shape_sums")
    table = np.frombuffer(sums, f3d._SHAPE_SUMS_DTYPE)
    pairs = [int(table["pairs"][:, k].sum()) for k in range(3)]
    if info.labelled != vox or not np.array_equal(table["n"], voxels.astype(np.uint64)) or pairs != equal:
        raise SystemExit(f"{name}: {info.as_dict()}, pairs {pairs} against {equal} equal neighbours counted by numpy")
    record(f"shape_{name}", 4, lambda: shape_fn(labels_dev, n, S, S, S, sums, C.byref(info)),
           {"labels": n, "built_s": round(built, 1), "copied_down_MB": round(n * 288 / 1e6, 1)})
    motion = (f3d.MotionSums * n)()
    record(f"label_sums_{name}", 16, lambda: label_sums_fn(*ins, labels_dev, n, 0, 0.0, S, S, S, motion, None))
    result[f"shape_{name}_over_label_sums"] = round(result[f"shape_{name}"]["ms"] / result[f"label_sums_{name}"]["ms"], 3)
    del motion
    if name != "random":
        found, capacity = f3d.ContactInfo(), 8 * n
        while True:                                                          # what OpticalFlowE::ComputeContacts does
            out = (f3d.Contact * capacity)()
            f3d.check(contacts_fn(0, 0, 0, labels_dev, n, S, S, S, capacity, out, C.byref(found)), "f3d_label_contacts")
            if found.complete:
                break
            capacity *= 2
        record(f"adjacency_{name}", 4, lambda: contacts_fn(0, 0, 0, labels_dev, n, S, S, S, capacity, out, C.byref(found)),
               {"capacity": capacity, "contacts": int(found.n_contacts)})
        result[f"shape_{name}_over_adjacency"] = round(result[f"shape_{name}"]["ms"] / result[f"adjacency_{name}"]["ms"], 3)
    t0 = time.perf_counter()
    shapes = f3d.solve_label_shapes(table)
    result[f"host_solve_ms_{name}"] = round((time.perf_counter() - t0) * 1e3, 2)
    result[f"euler_not_1_{name}"] = int((shapes.euler[shapes.status == 0] != 1).sum())
    print(json.dumps({k: v for k, v in result.items() if name in k}), flush=True)
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
        f.write(f"shape sums of labels at {S}^3, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls\n")
        f.write(f"{'call':<28}{'mean ms':>10}{'min ms':>10}{'B/voxel':>9}{'TB/s':>8}\n")
        for name, mean, best, need, rate in rows:
            f.write(f"{name:<28}{mean:>10.4f}{best:>10.4f}{need:>9}{rate:>8.3f}\n")
        for name, _ in cases:
            r = result[f"shape_{name}"]
            against = f", shape / adjacency {result[f'shape_{name}_over_adjacency']}" if f"shape_{name}_over_adjacency" in result else ""
            f.write(f"{name}: {r['labels']} labels, {r['copied_down_MB']} MB copied down, shape / f3d_label_motion_sums "
                    f"{result[f'shape_{name}_over_label_sums']}{against}, host solve {result[f'host_solve_ms_{name}']} ms, "
                    f"{result[f'euler_not_1_{name}']} bodies with Euler number != 1\n")
        if "bench" in result:
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        f"   (--gpus 1 --steps 3 --warmup 1, {S}^3)\n")
print(json.dumps(result), flush=True)
