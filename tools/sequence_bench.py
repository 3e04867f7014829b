#!/usr/bin/env python3
"""Frame-sequence throughput of bin/flow3d: N frames of one size written as RAW float32, then `flow3d --frames ...` twice --
pipelined (default: the next frame uploads and the previous flow downloads and is written beside the running solve) and with
F3D_SEQ_SERIAL=1 (the same work one step after the other), and with --concurrent 2 / 3 (that many pairs solved at once on lanes of
their own: what sequences of SMALL volumes want).   python tools/sequence_bench.py [--size 384] [--frames 6] [--concurrent 2 3]
--cumulative [--rounds R]: instead, what --cumulative (the displacement from frame 0 composed on the device and written beside the
flows) costs: pipelined runs without and with it, alternated R times, with the flow files of both compared.
--strain LIST [--rounds R]: the same for `--strain LIST` (e.g. vol,eq: the strain of each pair's flow computed on the device and
written beside it; add --cumulative for the strain of the displacement from frame 0, measured against --cumulative alone).
--principal LIST [--rounds R]: the same for `--principal LIST` (e.g. val,shear: the principal strains of each pair's flow)."""
import argparse
import importlib
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
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--concurrent", type=int, nargs="*", default=[2])
ap.add_argument("--cumulative", action="store_true")
ap.add_argument("--strain", default=None)
ap.add_argument("--principal", default=None)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
pkg = importlib.import_module("cuda-flow3d_amd")
S, N = a.size, a.frames
f0, f1 = pkg.synth_pair(S, S, S)
exe = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
    paths = []
    for k in range(N):
        t = k / max(1, N - 1)
        p = os.path.join(tmp, f"f{k}.raw")
        ((1 - t) * f0 + t * f1).astype(np.float32).tofile(p)
        paths.append(p)
    if a.cumulative or a.strain or a.principal:
        # A = the runs without the option measured, B = with it (--strain, --principal: both with --cumulative when it is given)
        field_option = ["--principal", a.principal] if a.principal else (["--strain", a.strain] if a.strain else None)
        base = ["--cumulative"] if a.cumulative and field_option else []
        b_tag = "principal" if a.principal else ("strain" if a.strain else "cumulative")
        extra = {"plain": base, b_tag: base + (field_option or ["--cumulative"])}
        walls = {"plain": [], b_tag: []}
        for r in range(a.rounds):
            for tag in ("plain", b_tag):
                t0 = time.time()
                run = subprocess.run([exe, "--dims", str(S), str(S), str(S), "--f32", "--frames", *paths, "--out", os.path.join(tmp, tag),
                                      "--silent"] + extra[tag], capture_output=True, text=True)
                wall = time.time() - t0
                walls[tag].append(wall / (N - 1))
                lost = re.findall(r"(\d+) of \d+ voxels have left the volume", run.stdout)
                folded = re.findall(r"(\d+) folded", run.stdout)
                print(f"round {r} {tag:10s} {S}^3 x {N} frames: wall {wall:.2f} s ({wall / (N - 1):.3f} s per pair), rc {run.returncode}"
                      + (f", lost per pair {lost}" if lost else "") + (f", folded per pair {folded}" if folded else ""), flush=True)
        same = all(open(os.path.join(tmp, f"{b_tag}_{k}_flow-{c}-{S}-{S}-{S}.raw"), "rb").read() ==
                   open(os.path.join(tmp, f"plain_{k}_flow-{c}-{S}-{S}-{S}.raw"), "rb").read() for k in range(N - 1) for c in "uvw")
        med = {k: sorted(v)[len(v) // 2] for k, v in walls.items()}
        print(f"median per pair: plain {med['plain']:.4f} s, {b_tag} {med[b_tag]:.4f} s "
              f"({100 * (med[b_tag] / med['plain'] - 1):+.2f} %); flows identical: {same}", flush=True)
        sys.exit(0)
    for tag, env in (("pipelined", {}), ("serial", {"F3D_SEQ_SERIAL": "1"})):
        t0 = time.time()
        run = subprocess.run([exe, "--dims", str(S), str(S), str(S), "--f32", "--frames", *paths, "--out", os.path.join(tmp, tag),
                              "--silent"], capture_output=True, text=True, env={**os.environ, **env})
        wall = time.time() - t0
        dev = [float(x) for x in re.findall(r"pair \d+ of \d+: ([\d.]+) s on the device", run.stdout)]
        print(f"{tag:10s} {S}^3 x {N} frames: wall {wall:.2f} s, device {sum(dev):.2f} s over {len(dev)} pairs "
              f"({wall / max(1, len(dev)):.3f} s per pair), rc {run.returncode}", flush=True)
    for n in a.concurrent:
        t0 = time.time()
        run = subprocess.run([exe, "--dims", str(S), str(S), str(S), "--f32", "--frames", *paths, "--out", os.path.join(tmp, f"c{n}"),
                              "--silent", "--concurrent", str(n)], capture_output=True, text=True)
        wall = time.time() - t0
        m = re.search(r"(\d+) pairs in ([\d.]+) s: ([\d.]+) pairs per second", run.stdout)
        print(f"concurrent {n}: {S}^3 x {N} frames: wall {wall:.2f} s, " + (f"{m.group(1)} pairs in {m.group(2)} s = {float(m.group(2)) / int(m.group(1)):.3f} s per pair"
              if m else "no summary line") + f", rc {run.returncode}", flush=True)
        if n == a.concurrent[0]:   # the same bits as the pipelined run
            same = all(open(os.path.join(tmp, f"c{n}_{k}_flow-{c}-{S}-{S}-{S}.raw"), "rb").read() ==
                       open(os.path.join(tmp, f"pipelined_{k}_flow-{c}-{S}-{S}-{S}.raw"), "rb").read() for k in range(N - 1) for c in "uvw")
            print(f"concurrent {n}: results identical to the pipelined run: {same}", flush=True)
