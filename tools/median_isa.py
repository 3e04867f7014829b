#!/usr/bin/env python3
"""Resource report and instruction counts of the median kernels, read from the gfx950 assembly that the Makefile's flags for
f3d_median.hip give (make asm-median).  Runs on the CPU: hipcc only cross-compiles.

    python tools/median_isa.py                 one line per median kernel
    python tools/median_isa.py --asm FILE      the same for an assembly file that already exists

Per kernel: VGPRs, LDS bytes, scratch bytes, waves per SIMD, vector instructions, v_min/v_max(3)_f32 among them, and the
self-canonicalising `v_max_f32 vN, vN, vN` that the compiler puts in front of an IEEE fminf / fmaxf of a value it cannot prove
quiet (none are wanted: the median reads in-box voxels only).  The counts are static: a loop body counts once, so the march of
k_median_keep (three steps unrolled) and k_median_share (four steps unrolled) divide by their unroll depth after taking off the
chunk prologue.
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANON = re.compile(r"v_max_f32(?:_e32|_e64)?\s+(v\d+), \1, \1\s*$")
MINMAX = re.compile(r"v_(?:min|max)3?_f32")


def compile_to_asm():
    out = os.path.join(tempfile.mkdtemp(prefix="f3d_median_isa_"), "f3d_median.s")
    subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "--no-print-directory", "asm-median", "ASM_OUT=" + out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """{mangled name: {"body": [instructions], "vgprs", "lds", "scratch", "occupancy"}}"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), {"body": []})
            continue
        if cur is None:
            continue
        text = line.split(";")[0].strip()
        for key, pat in (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("lds", r";\s*LDSByteSize:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)"),
                         ("occupancy", r";\s*Occupancy:\s*(\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
        if text and not text.startswith(".") and not text.endswith(":") and "occupancy" not in cur:
            cur["body"].append(text)
    return out


def report(path=None):
    """{short kernel name: dict of figures} for every kernel of f3d_median.hip"""
    res = {}
    for name, k in kernels(path or compile_to_asm()).items():
        m = re.search(r"(k_median_[a-z]+)(?:ILi(\d+)E)?", name)
        if not m or "occupancy" not in k:
            continue
        ops = [t.split()[0] for t in k["body"]]
        res[m.group(1) + (f"<{m.group(2)}>" if m.group(2) else "")] = dict(
            vgprs=k["vgprs"], lds=k["lds"], scratch=k["scratch"], waves_per_simd=k["occupancy"],
            valu=sum(o.startswith("v_") for o in ops), minmax=sum(bool(MINMAX.match(o)) for o in ops),
            canonicalise=sum(bool(CANON.match(t)) for t in k["body"]), barriers=ops.count("s_barrier"),
            lds_ops=sum(o.startswith("ds_") for o in ops))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="an assembly file of f3d_median.hip instead of compiling one")
    for name, fig in sorted(report(ap.parse_args().asm).items()):
        print(f"{name:20s}", " ".join(f"{k}={v}" for k, v in fig.items()))
