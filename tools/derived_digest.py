#!/usr/bin/env python3
"""Digests of what the derived-field entry points of the loaded device library compute, for comparing two builds byte for byte
(F3D_LIBDIR names the other one): f3d_flow_strain and f3d_principal_strain with every group, f3d_invert_displacement,
f3d_carry_field in both modes and f3d_compose_flow, on the flow of the synthetic pair at --size^3 and on a 70 x 9 x 20 box (no
multiple of the 64 x 4 x 32 tiles) of a seeded smooth displacement with NaN planted.  One line per array (sha256 of its bytes) and
per statistics field (its bits in hex), so `diff` of two runs names what moved.
    python tools/derived_digest.py [--size 128]"""
import argparse
import hashlib
import importlib
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=128)
a = ap.parse_args()
f3d = importlib.import_module("cuda-flow3d_amd")


def show(case, name, value):
    if isinstance(value, np.ndarray):
        print(f"{case} {name} sha256 {hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest()}")
    elif isinstance(value, float):
        print(f"{case} {name} bits {struct.pack('<d', value).hex()}")   # a float32 statistic widens exactly
    else:
        print(f"{case} {name} value {int(value)}")


def run(case, field, disp):
    for n, c in zip("uvw", disp):
        show(case, "input_" + n, c)
    for label, res in (("strain", f3d.flow_strain(*disp, fields=("vol", "e", "eq"))),
                       ("principal", f3d.principal_strain(*disp, fields=("val", "shear", "dir1", "dir3")))):
        stats = res.pop("stats")
        for n, v in res.items():
            show(case, f"{label}_{n}", v)
        for n, v in stats.items():
            show(case, f"{label}_stats_{n}", v)
    *inv, stats = f3d.invert_displacement(*disp)
    for n, v in zip(f3d.INVERSE_NAMES, inv):
        show(case, "inverse_" + n, v)
    for n, v in stats.items():
        show(case, "inverse_stats_" + n, v)
    for mode in f3d.CARRY_MODES:
        out, lost = f3d.carry_field(field, *inv[:3], mode=mode)
        show(case, f"carry_{mode}", out)
        show(case, f"carry_{mode}_lost", lost)
    *acc, lost = f3d.compose_flow(disp, disp)
    for n, v in zip("uvw", acc):
        show(case, "compose_" + n, v)
    show(case, "compose_lost", lost)


S = a.size
f0, f1 = f3d.synth_pair(S, S, S)
flow = f3d.OpticalFlow()
flow.initialize(S, S, S)
uvw = flow.compute(f0, f1, silent=True, warp_levels_count=6, outer_iterations_count=4, inner_iterations_count=5)
flow.destroy()
run(f"pair{S}", f0, [np.ascontiguousarray(c, dtype=np.float32) for c in uvw])

W, H, D = 70, 9, 20
rng = np.random.default_rng(7)
z, y, x = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
disp = [(np.float32(2.5) * np.sin(x / 11 + k) * np.cos(y / 5 - k) * np.sin(z / 7 + 2 * k)
         + np.float32(0.05) * rng.standard_normal(size=(D, H, W), dtype=np.float32)).astype(np.float32) for k in range(3)]
for c in disp:
    c[rng.random(size=(D, H, W)) < 0.03] = np.nan
run("box70x9x20", rng.random(size=(D, H, W), dtype=np.float32), disp)
