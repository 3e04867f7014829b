#!/usr/bin/env python3
"""Time of the exact nearest-seed transform (f3d_nearest_seed) and of the split of touching bodies (f3d_split_components) at --size^3 on
three inputs, --reps calls per row between HIP events round the whole blocking entry (the clearing of the counters, every kernel, the
copy of the counters down and the wait included) after --warmup calls:
    cells    Voronoi cells of about --cell voxels across (tools/contacts_bench.py's, 5 832 at 512^3) with their one-voxel walls set to
             background: thousands of compact bodies, short lines everywhere
    pore     one solid block with a single background voxel in the middle: the linear-work check.  Every line of the distance to the
             background carries one parabola or none; a search outward from every voxel would be quadratic here
    noise    uniform noise thresholded at p = 0.31: a seed every few voxels, the deepest stacks
Per input, in the same invocation: f3d_nearest_seed in mode F3D_SEED_ZERO (the distance to the background) with d2_out alone and with
all three outputs, f3d_split_components at --core-d2, and as the yardstick f3d_label_components, which is existing code.
The host route (download, scipy.ndimage.distance_transform_edt, upload) is run once, on the first input, for orientation, and its
squared and rounded distances are compared with d2_out (--skip-host leaves it out, for a run under a profiler).
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Prints one JSON line.
    python tools/nearest_bench.py [--size 512] [--cell 30] [--core-d2 49] [--reps 5] [--warmup 1] [--table PATH] [--skip-host]"""
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
ap.add_argument("--core-d2", type=int, default=49)
ap.add_argument("--min-voxels", type=int, default=27)
ap.add_argument("--table")
ap.add_argument("--parent-libdir")
ap.add_argument("--skip-host", action="store_true")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S = a.size
vox = S ** 3
rng = np.random.default_rng(0)


def cells(size, across):
    """tools/contacts_bench.py's label volume: labels 1 .. g^3 of the nearest of g^3 seeds jittered on a grid of pitch `across`, at half
    the size and doubled along each axis"""
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


def without_walls(labels):
    """1.0 inside a cell, 0.0 where a voxel differs from its +x, +y or +z neighbour"""
    wall = np.zeros(labels.shape, bool)
    wall[:, :, :-1] |= labels[:, :, :-1] != labels[:, :, 1:]
    wall[:, :-1, :] |= labels[:, :-1, :] != labels[:, 1:, :]
    wall[:-1, :, :] |= labels[:-1, :, :] != labels[1:, :, :]
    return (~wall).astype(np.float32)


components_fn = f3d._components_entry()
nearest_fn = f3d._nearest_entry()
split_fn = f3d._split_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
src = box.alloc()
labels_dev = box.alloc()
d2_dev, index_dev, value_dev = box.alloc(), box.alloc(), box.alloc()
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


result = {"size": S, "reps": a.reps, "core_d2": a.core_d2, "min_voxels": a.min_voxels}
rows = []


def record(name, call, extra=None):
    mean, best = timed(name, call)
    result[name] = {"ms": round(mean, 4), "min_ms": round(best, 4)}
    if extra:
        result[name].update(extra)
    rows.append((name, mean, best))




def pore():
    volume = np.ones((S, S, S), np.float32)
    volume[S // 2, S // 2, S // 2] = 0
    return volume


cases = [("cells", lambda: without_walls(cells(S, a.cell)[0])), ("pore", pore),
         ("noise", lambda: (rng.random((S, S, S), dtype=np.float32) < np.float32(0.31)).astype(np.float32))]
for at, (name, make) in enumerate(cases):
    t0 = time.perf_counter()
    volume = make()
    built = time.perf_counter() - t0
    box.upload(src, volume)                                              # 1.0f and 0.0f: non-zero and zero as int32 too
    near = f3d.NearestInfo()
    record(f"nearest_d2_{name}", lambda: nearest_fn(src, f3d.SEED_MODES["zero"], 0, d2_dev, 0, 0, S, S, S, C.byref(near)),
           {"built_s": round(built, 1)})
    record(f"nearest_all_{name}", lambda: nearest_fn(src, f3d.SEED_MODES["zero"], 0, d2_dev, index_dev, value_dev, S, S, S, C.byref(near)))
    result[f"nearest_all_{name}"].update(near.as_dict())
    split = f3d.SplitInfo()
    record(f"split_{name}", lambda: split_fn(src, 0.5, 1.5, a.core_d2, a.min_voxels, labels_dev, S, S, S, None, 0, C.byref(split)))
    result[f"split_{name}"].update(split.as_dict())
    info = f3d.ComponentInfo()
    record(f"components_{name}", lambda: components_fn(src, 0.5, 1.5, a.min_voxels, labels_dev, S, S, S, None, 0, C.byref(info)))
    result[f"components_{name}"].update(info.as_dict())
    for which in ("nearest_d2", "nearest_all", "split"):
        result[f"{which}_{name}_over_components"] = round(result[f"{which}_{name}"]["ms"] / result[f"components_{name}"]["ms"], 3)
    if near.seeds != vox - info.foreground or split.foreground != info.foreground:
        raise SystemExit(f"{name}: {near.as_dict()} and {split.as_dict()} against {info.as_dict()}")
    if not a.skip_host and at == 0:
        from scipy import ndimage
        t0 = time.perf_counter()
        down = box.download(src, (S, S, S))
        t1 = time.perf_counter()
        edt = ndimage.distance_transform_edt(down != 0)
        t2 = time.perf_counter()
        box.upload(labels_dev, edt.astype(np.float32))
        t3 = time.perf_counter()
        result[f"host_{name}"] = {"download_ms": round((t1 - t0) * 1e3, 1), "scipy_edt_ms": round((t2 - t1) * 1e3, 1),
                                  "upload_ms": round((t3 - t2) * 1e3, 1)}
        got = box.download(d2_dev, (S, S, S)).view(np.int32)
        if not np.array_equal(got, np.rint(edt * edt).astype(np.int32)):
            raise SystemExit(f"{name}: d2_out differs from scipy.ndimage.distance_transform_edt squared")
        del down, edt, got
    del volume
    print(json.dumps({k: v for k, v in result.items() if k.endswith(name) or f"_{name}_" in k}), flush=True)
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
        f.write(f"nearest seed and split at {S}^3, core_d2 {a.core_d2}, min_voxels {a.min_voxels}, {a.reps} calls per row between HIP events "
                f"after {a.warmup} warm-up calls\n")
        f.write(f"{'call':<28}{'mean ms':>10}{'min ms':>10}{'ns/voxel':>10}\n")
        for name, mean, best in rows:
            f.write(f"{name:<28}{mean:>10.4f}{best:>10.4f}{mean * 1e6 / vox:>10.4f}\n")
        for name, _ in cases:
            n, s_, c = result[f"nearest_all_{name}"], result[f"split_{name}"], result[f"components_{name}"]
            f.write(f"{name}: {n['seeds']} background voxels, d2_max {n['d2_max']}; {c['n_components']} components -> "
                    f"{s_['n_cores']} cores, {s_['remainder_bodies']} remainder bodies of {s_['remainder_voxels']} voxels, {s_['n_labels']} labels; "
                    f"nearest (d2) / nearest (all) / split over f3d_label_components "
                    f"{result[f'nearest_d2_{name}_over_components']} / {result[f'nearest_all_{name}_over_components']} / "
                    f"{result[f'split_{name}_over_components']}")
            if f"host_{name}" in result:
                h = result[f"host_{name}"]
                f.write(f"; host: download {h['download_ms']} ms, scipy.ndimage.distance_transform_edt {h['scipy_edt_ms']} ms, upload {h['upload_ms']} ms")
            f.write("\n")
        if "bench" in result:
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        f"   (--gpus 1 --steps 3 --warmup 1, {S}^3)\n")
print(json.dumps(result), flush=True)
