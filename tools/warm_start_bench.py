#!/usr/bin/env python3
"""The two routes to the displacement from frame 0 of a sequence, on the same frames in one invocation: `flow3d --cumulative` at the
default depth (consecutive pairs, composed on the device) against `flow3d --total --levels L` for a few depths L (frame 0 -> frame
k+1 solved directly, started from the pair before).  The frames are three Gaussian blobs and a ripple, translated by k * --step
voxels in frame k, so the displacement from frame 0 is known everywhere: N frames of --size^3 written as RAW float32.  Reports the
seconds per pair on the device, the wall seconds per pair of the whole run (start-up, files and the host's waits included; a plain
run and a --warm-start run give the yardstick) and the rms of the vector error of the displacement frame 0 -> last frame over the interior (a margin
of the largest displacement plus 16 voxels; voxels that are NaN -- lost under --cumulative -- are counted and left out).
Then the time of one f3d_initial_flow (k_initial_flow, the preparation of a solve's start) at --kernel-size^3: HIP events round the
blocking entry, five calls after one warm-up.
    --table PATH         writes the text table
    --parent-libdir DIR  also runs bench.py twice on this build and twice on the libraries in DIR (F3D_LIBDIR), alternating, in
                         child processes of their own, to show that the solve did not move
Prints one JSON line.
    python tools/warm_start_bench.py [--size 384] [--frames 5] [--step 3 -2 1.5] [--levels 40 20 10 5] [--kernel-size 512]"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=384)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--step", type=float, nargs=3, default=[3.0, -2.0, 1.5])
ap.add_argument("--levels", type=int, nargs="*", default=[40, 20, 10, 5])
ap.add_argument("--kernel-size", type=int, default=512)
ap.add_argument("--table")
ap.add_argument("--parent-libdir")
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")
S, N = a.size, a.frames
exe = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")


def frame(shift):
    """three blobs and a ripple translated by `shift` (x, y, z): every term is a product of functions of one axis"""
    axes = [np.arange(S, dtype=np.float64) - s for s in shift]   # x', y', z'

    def separable(fx, fy, fz):
        return (fz(axes[2])[:, None, None] * fy(axes[1])[None, :, None] * fx(axes[0])[None, None, :]).astype(np.float32)

    def blob(c, sigma):
        return separable(*[lambda t, m=m: np.exp(-((t - m) ** 2) / (2.0 * sigma ** 2)) for m in c])

    img = 180.0 * blob((0.4 * S, 0.5 * S, 0.5 * S), S / 7.0) + 90.0 * blob((0.7 * S, 0.3 * S, 0.4 * S), S / 10.0)
    img += 70.0 * blob((0.3 * S, 0.75 * S, 0.6 * S), S / 9.0)
    k = 48.0 / S   # the ripple of the 48-voxel test pair, stretched with the volume
    img += 25.0 * separable(lambda t: np.sin(0.45 * k * t), lambda t: np.cos(0.4 * k * t), lambda t: np.cos(0.5 * k * t))
    return img.astype(np.float32)


truth = [(N - 1) * s for s in a.step]
margin = int(np.ceil(max(abs(t) for t in truth))) + 16


def error_of(prefix, kind):
    comps = [np.fromfile(f"{prefix}_{N - 2}_{kind}-{c}-{S}-{S}-{S}.raw", np.float32).reshape(S, S, S)[margin:-margin, margin:-margin, margin:-margin]
             for c in "uvw"]
    e = sum((c.astype(np.float64) - t) ** 2 for c, t in zip(comps, truth))
    lost = int(np.isnan(e).sum())
    return float(np.sqrt(np.nanmean(e))), lost


result = {"size": S, "frames": N, "step": a.step, "truth_last": truth, "margin": margin, "rows": []}
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
    paths = []
    for k in range(N):
        p = os.path.join(tmp, f"f{k}.raw")
        frame([k * s for s in a.step]).tofile(p)
        paths.append(p)
    # plain and --warm-start write what --total writes (three flow files per pair): their wall seconds show what preparing the start
    # costs the host, which waits for the library stream to read the info line before it issues the solve (the device timer starts
    # after that wait); --cumulative writes three more files per pair
    runs = [("plain", [], None), ("warm-start", ["--warm-start"], None), ("cumulative", ["--cumulative"], "disp")]
    runs += [(f"total L={L}", ["--total", "--levels", str(L)], "flow") for L in a.levels]
    for tag, extra, kind in runs:
        prefix = os.path.join(tmp, tag.replace(" ", "_").replace("=", ""))
        t0 = time.time()
        run = subprocess.run([exe, "--dims", str(S), str(S), str(S), "--f32", "--frames", *paths, "--out", prefix, "--silent"] + extra,
                             capture_output=True, text=True)
        dev = [float(x) for x in re.findall(r"pair \d+ of \d+: ([\d.]+) s on the device", run.stdout)]
        if run.returncode != 0 or len(dev) != N - 1:
            raise SystemExit(f"flow3d {tag} failed (rc {run.returncode}): {run.stdout[-800:]} {run.stderr[-800:]}")
        wall = (time.time() - t0) / (N - 1)
        rms, lost = error_of(prefix, kind) if kind else (float("nan"), 0)
        found = re.findall(r"initial flow: (\d+) replaced, (\d+) leaving, max \|\.\| ([-\d.e+]+)", run.stdout)
        row = {"run": tag, "device_s_per_pair": [round(x, 4) for x in dev], "mean_device_s_per_pair": round(sum(dev) / len(dev), 4), "wall_s_per_pair": round(wall, 4),
               "rms_error_last": round(rms, 5), "nan_in_interior": lost, "initial": found}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

# ---- the preparation kernel ----
K = a.kernel_size
fn = f3d._initial_entry()
hip = f3d.hip()
box = f3d.Containers(K, K, K)
ptrs = [box.new(fill=0) for _ in range(3)]
box.set_current()
info = f3d.InitialInfo()
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    f3d.check(hip.f3d_event_create(C.byref(e)))
times = []
for i in range(6):
    f3d.check(hip.f3d_event_record(ev[0]))
    f3d.check(fn(*ptrs, *ptrs, K, K, K, C.byref(info)), "f3d_initial_flow")
    f3d.check(hip.f3d_event_record(ev[1]))
    f3d.check(hip.f3d_event_sync(ev[1]))
    ms = C.c_float()
    f3d.check(hip.f3d_event_elapsed_ms(C.byref(ms), ev[0], ev[1]))
    if i:
        times.append(ms.value)
for e in ev:
    hip.f3d_event_destroy(e)
box.free()
result["k_initial_flow"] = {"size": K, "ms": [round(t, 4) for t in times], "mean_ms": round(sum(times) / len(times), 4),
                            "TB_per_s_at_24_B_per_voxel": round(24.0 * K ** 3 / (min(times) * 1e-3) / 1e12, 3)}

if a.parent_libdir:
    # the solve against the parent's libraries, alternating, every run a fresh process
    bench = {"this": [], "parent": []}
    for which in ("this", "parent", "this", "parent"):
        env = dict(os.environ)
        if which == "parent":
            env["F3D_LIBDIR"] = os.path.abspath(a.parent_libdir)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env,
                           capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not line:
            raise SystemExit(f"bench.py ({which}) failed: {p.stdout[-500:]} {p.stderr[-1500:]}")
        bench[which].append(json.loads(line[-1]))
    result["bench"] = bench

if a.table:
    with open(a.table, "w") as f:
        f.write(f"displacement frame 0 -> frame {N - 1} of {N} frames of {S}^3 moving by {tuple(a.step)} voxels per frame (truth {tuple(truth)}); "
                f"rms of the vector error over the interior (margin {margin})\n")
        f.write(f"{'run':<16}{'s per pair (device)':>22}{'s per pair (wall)':>20}{'rms error':>12}{'NaN':>8}   per pair\n")
        for r in result["rows"]:
            f.write(f"{r['run']:<16}{r['mean_device_s_per_pair']:>22.4f}{r['wall_s_per_pair']:>20.4f}{r['rms_error_last']:>12.5f}{r['nan_in_interior']:>8}   {r['device_s_per_pair']}\n")
        ki = result["k_initial_flow"]
        f.write(f"k_initial_flow at {K}^3, in place, with info (blocking entry between HIP events, 5 calls after 1 warm-up): mean {ki['mean_ms']} ms, "
                f"{ki['ms']}; best = {ki['TB_per_s_at_24_B_per_voxel']} TB/s at 24 B per voxel\n")
        if "bench" in result:
            for which, runs_ in result["bench"].items():
                f.write(f"bench.py {which}: " + ", ".join(f"{r['value']} {r['unit']} ({r['ms_per_step']} ms per step)" for r in runs_) +
                        "   (--gpus 1 --steps 3 --warmup 1)\n")
print(json.dumps(result), flush=True)
