#!/usr/bin/env python3
"""Time of the connected bodies of a thresholded volume (f3d_label_components) at --size^3 on three inputs, --reps calls per row between
HIP events round the whole blocking entry (the clearing of the counters, every kernel, the copy of the counters down and the wait
included) after --warmup calls:
    full     every voxel foreground: one body, the longest chains of parents
    cells    Voronoi cells of about --cell voxels across (tools/contacts_bench.py's, 5 832 at 512^3) with their one-voxel walls set to
             background: thousands of compact bodies
    noise    uniform noise thresholded at p = 0.31, the site-percolation threshold of the cubic lattice: tortuous clusters across many
             tiles and millions of bodies
In the same invocation, as the yardstick, f3d_label_motion_sums without a weight on the labels the call just made (with a displacement
of seeded noise, whose values do not matter to the time); labels beyond its limit of 2^22 are foreign to it, which costs it nothing.
n_components of every input is checked against scipy.ndimage.label, whose time on the host, and the download and upload a host
labelling implies, are given for orientation (--skip-host leaves all that out, for a run under a profiler).
    --table PATH         also writes the numbers as a text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Prints one JSON line.
    python tools/components_bench.py [--size 512] [--cell 30] [--reps 5] [--warmup 1] [--min-voxels 27] [--table PATH] [--skip-host]"""
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
label_sums_fn, _ = f3d._label_motion_entry()
hip = f3d.hip()
box = f3d.Containers(S, S, S)
disp = [box.new(rng.standard_normal((S, S, S), dtype=np.float32) * np.float32(0.5) + np.float32(m)) for m in (2.0, -1.0, 0.5)]
src = box.alloc()
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


result = {"size": S, "reps": a.reps, "min_voxels": a.min_voxels}
rows = []


def record(name, call, extra=None):
    mean, best = timed(name, call)
    result[name] = {"ms": round(mean, 4), "min_ms": round(best, 4)}
    if extra:
        result[name].update(extra)
    rows.append((name, mean, best))


cases = [("full", lambda: np.ones((S, S, S), np.float32)), ("cells", lambda: without_walls(cells(S, a.cell)[0])),
         ("noise", lambda: (rng.random((S, S, S), dtype=np.float32) < np.float32(0.31)).astype(np.float32))]
for name, make in cases:
    t0 = time.perf_counter()
    volume = make()
    built = time.perf_counter() - t0
    box.upload(src, volume)
    info = f3d.ComponentInfo()
    record(f"components_{name}", lambda: components_fn(src, 0.5, 1.5, a.min_voxels, labels_dev, S, S, S, None, 0, C.byref(info)),
           {"built_s": round(built, 1)})
    result[f"components_{name}"].update(info.as_dict())
    n = max(1, min(int(info.n_labels), f3d.MAX_LABELS))
    sums = (f3d.MotionSums * n)()
    record(f"label_sums_{name}", lambda: label_sums_fn(*disp, labels_dev, n, 0, 0.0, S, S, S, sums, None), {"labels": n})
    result[f"components_{name}_over_label_sums"] = round(result[f"components_{name}"]["ms"] / result[f"label_sums_{name}"]["ms"], 3)
    if not a.skip_host:
        from scipy import ndimage
        t0 = time.perf_counter()
        down = box.download(src, (S, S, S))
        t1 = time.perf_counter()
        found, count = ndimage.label(down >= 0.5)
        t2 = time.perf_counter()
        box.upload(labels_dev, found.astype(np.int32).view(np.float32))
        t3 = time.perf_counter()
        result[f"host_{name}"] = {"download_ms": round((t1 - t0) * 1e3, 1), "scipy_label_ms": round((t2 - t1) * 1e3, 1),
                                  "upload_ms": round((t3 - t2) * 1e3, 1), "components": int(count)}
        if count != info.n_components or int((found > 0).sum()) != info.foreground:
            raise SystemExit(f"{name}: {info.as_dict()} against {count} components counted by scipy.ndimage.label")
        del down, found
    del volume
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
        f.write(f"connected bodies at {S}^3, min_voxels {a.min_voxels}, {a.reps} calls per row between HIP events after {a.warmup} warm-up calls\n")
        f.write(f"{'call':<28}{'mean ms':>10}{'min ms':>10}\n")
        for name, mean, best in rows:
            f.write(f"{name:<28}{mean:>10.4f}{best:>10.4f}\n")
        for name, _ in cases:
            r = result[f"components_{name}"]
            f.write(f"{name}: {r['n_components']} components, {r['n_labels']} labels, largest {r['largest']}, {r['foreground']} foreground; "
                    f"components / f3d_label_motion_sums {result[f'components_{name}_over_label_sums']}")
            if f"host_{name}" in result:
                h = result[f"host_{name}"]
                f.write(f"; host: download {h['download_ms']} ms, scipy.ndimage.label {h['scipy_label_ms']} ms, upload {h['upload_ms']} ms")
            f.write("\n")
        if "bench" in result:
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        f"   (--gpus 1 --steps 3 --warmup 1, {S}^3)\n")
print(json.dumps(result), flush=True)
