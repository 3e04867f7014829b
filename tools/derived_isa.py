#!/usr/bin/env python3
"""Resource report and instruction counts of the derived-field kernels (strain, principal strain, polar decomposition, inverse / carry, trajectory),
read from the gfx950 assembly that the Makefile's flags give.  Runs on the CPU: hipcc only cross-compiles.

    python tools/derived_isa.py                     one line per kernel of this tree
    python tools/derived_isa.py --tree DIR          the same for another checkout (a parent commit, say)
    python tools/derived_isa.py --against DIR       this tree next to DIR: the kernels whose figures differ, with their opcode diffs

Per kernel: VGPRs, LDS bytes, scratch bytes, waves per SIMD, global loads, global stores, ds_* instructions, s_barrier, cross-lane
instructions (DPP modifiers, v_permlane*, ds_bpermute / ds_permute / ds_swizzle), the number of instructions, and a digest of the
instruction sequence with every register renamed in order of first appearance and every label dropped, so two compilations that
differ only in register allocation or label numbering have the same digest.  The counts are static: a loop body counts once.
"""
import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # so that it also runs as a module or from another directory
from median_isa import kernels  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("f3d_strain", "f3d_principal", "f3d_polar", "f3d_inverse", "f3d_trajectory")
FIGURES = ("vgprs", "lds", "scratch", "occupancy", "global_loads", "global_stores", "ds", "barriers", "cross_lane")
CROSS = re.compile(r"\b(row_|quad_perm|wave_sh|wave_ro|bank_mask|v_permlane|ds_bpermute|ds_permute|ds_swizzle)")


def compiler(tree):
    """[HIPCC, *HIPFLAGS] of the tree's Makefile, as make expands them"""
    out = subprocess.run(["make", "-C", os.path.join(tree, "cuda-flow3d_amd"), "--no-print-directory", "-pn"], check=True,
                         capture_output=True, text=True).stdout
    found = {}
    for var in ("HIPCC", "HIPFLAGS"):
        m = re.search(rf"^{var}\s*[:?+]?=\s*(.*)$", out, re.M)
        if not m:
            raise SystemExit(f"{tree}/cuda-flow3d_amd/Makefile: no {var} assignment in `make -pn`")
        found[var] = m.group(1).split()
    return found["HIPCC"] + found["HIPFLAGS"]


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return [re.sub(r"\(anonymous namespace\)::|f3d_partials::|\(.*$|^void ", "", line) for line in out.splitlines()]


def digest(body):
    seen = {}

    def rename(m):
        return seen.setdefault(m.group(0), f"{m.group(1)}#{len(seen)}")

    text = "\n".join(re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", rename, re.sub(r"\.?LBB\d+_\d+", "L", t)) for t in body)
    return hashlib.sha256(text.encode()).hexdigest()[:12]


def report(tree=ROOT):
    """{kernel: {figure: value}} of the device files of a tree (those of FILES that it has: an older checkout lacks the newer ones)"""
    res = {}
    with tempfile.TemporaryDirectory(prefix="f3d_derived_isa_") as tmp:
        for f in FILES:
            src = os.path.join(tree, "cuda-flow3d_amd", "csrc", f + ".hip")
            if not os.path.exists(src):
                continue
            asm = os.path.join(tmp, f + ".s")
            subprocess.run([*compiler(tree), "-S", "--cuda-device-only", src, "-o", asm], check=True)
            ks = {n: k for n, k in kernels(asm).items() if "occupancy" in k}
            for name, k in zip(demangled(list(ks)), ks.values()):
                ops = [t.split()[0] for t in k["body"]]
                res[name] = dict(
                    file=f, vgprs=k["vgprs"], lds=k["lds"], scratch=k["scratch"], occupancy=k["occupancy"],
                    global_loads=sum(o.startswith(("global_load", "flat_load", "buffer_load")) for o in ops),
                    global_stores=sum(o.startswith(("global_store", "flat_store", "buffer_store")) for o in ops),
                    ds=sum(o.startswith("ds_") for o in ops), barriers=ops.count("s_barrier"),
                    cross_lane=sum(bool(CROSS.search(t)) for t in k["body"]), instructions=len(ops), sequence=digest(k["body"]),
                    ops=collections.Counter(ops))
    return res


def line(name, fig):
    return f"{name:44s} " + " ".join(f"{k}={v}" for k, v in fig.items() if k not in ("ops", "file"))


def by_role(rep):
    """the fold kernel of a file under one key, whatever it is called (k_*_stats before they became fold_partials<P>)"""
    return {(fig["file"] + " fold" if "fold_partials" in name or name.endswith("_stats") else name): (name, fig)
            for name, fig in rep.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout to report (default: this one)")
    ap.add_argument("--against", help="a second checkout to compare this one with")
    args = ap.parse_args()
    mine = report(args.tree)
    for name, fig in sorted(mine.items()):
        print(line(name, fig))
    if args.against:
        theirs = report(args.against)
        print("\nthe tree compared against:")
        for name, fig in sorted(theirs.items()):
            print(line(name, fig))
        print("\ndifferences (a file's fold kernel is matched whatever its name):")
        mine, theirs = by_role(mine), by_role(theirs)
        for key in sorted(set(mine) | set(theirs)):
            if key not in mine or key not in theirs:
                print(f"  {key}: only in {'this tree' if key in mine else 'the tree compared against'}")
                continue
            (a, x), (b, y) = mine[key], theirs[key]
            moved = [k for k in FIGURES if x[k] != y[k]]
            if moved or x["sequence"] != y["sequence"]:
                ops = {o: x["ops"][o] - y["ops"][o] for o in sorted(set(x["ops"]) | set(y["ops"])) if x["ops"][o] != y["ops"][o]}
                print(f"  {a} / {b}: figures {moved or 'equal'}, sequence {'equal' if x['sequence'] == y['sequence'] else 'differs'}, "
                      f"opcode counts {ops or 'equal'}")
        print("  (end)")
