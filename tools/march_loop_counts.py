#!/usr/bin/env python3
"""Static instruction counts of the steady march loop of the fused solver kernels (k_pair8 / k_wpair8), from device assembly.

The march of a row wave is unrolled three steps deep: in the assembly it is the region between a label and a backward branch to that
label that holds exactly three `s_barrier` and the hand-issued `global_store_dword` of the owned rows (the column wave's loop has the
barriers but stores nothing; the loader's loop issues DMA pieces).  A build that folds (FOLDS) has two such loops, one per tile kind.
The region only finds the loop: what is counted are all blocks the compiler marks as members of that loop, wherever it laid them out,
so the cold blocks (IEEE fallbacks) are counted too: `VALU` is everything that starts with v_, divide by three for a step.  A record of
what a change moved, not a check.

  python3 tools/march_loop_counts.py [file.s] [--kernels k_wpair8ILi2 k_pair8ILi0ELi12ELi0ELb1]
Without a file the solver source is compiled with the product's flags (as tools/isa_hazards.py does)."""
import argparse
import collections
import re
import sys

COLUMNS = (("VALU", r"v_"), ("v_mov_b32", r"v_mov_b32(_e32|_e64)?$"), ("v_mov_b32_dpp", r"v_mov_b32_dpp$"),
           ("v_readlane_b32", r"v_readlane_b32$"), ("v_readfirstlane_b32", r"v_readfirstlane_b32$"), ("s_nop", r"s_nop$"),
           ("s_cbranch_vccnz", r"s_cbranch_vccn?z$"), ("f64", r"v_\w*f64"), ("v_lshl_add_u32", r"v_lshl_add_u32$"),
           ("v_min3_u32", r"v_min3_u32$"), ("v_div_fixup_f32", r"v_div_fixup_f32$"), ("v_cndmask_b32", r"v_cndmask_b32"),
           ("SALU", r"s_(?!nop|barrier|waitcnt|cbranch|branch)"), ("ds_read", r"ds_read"), ("ds_write", r"ds_write"))


def functions(path, keys):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = (m.group(1), []) if any(k in m.group(1) for k in keys) else (None, [])
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        body.append(line.rstrip("\n"))


def march_loops(body):
    """(first line, last line) of every backward-branch region with three barriers and stores"""
    labels = {}
    for i, line in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            labels[m.group(1)] = i
    found = []
    for i, line in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", line)
        if not m or labels.get(m.group(1), i) >= i:
            continue
        lo = labels[m.group(1)]
        region = body[lo:i + 1]
        if sum(1 for l in region if re.match(r"^\s+s_barrier", l)) == 3 and any("global_store_dword" in l for l in region):
            found.append((lo, i))
    # the remainder steps branch back as well: of nested regions keep the innermost
    return [(lo, hi) for lo, hi in found if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in found)]


def loop_blocks(body, lo):
    """every line of the loop whose header is the label on line `lo`, wherever the assembler laid its blocks out: the compiler marks each
    block `in Loop: Header=BBn_m` (inner loops: `Parent Loop BBn_m`)"""
    m = re.search(r"Header=(BB\w+)", body[lo])      # (the branch target need not be the header: a latch can be laid out in front of it)
    head = m.group(1) if m else re.match(r"^\.L(BB\w+):", body[lo]).group(1)
    inside, out = False, []
    for i, line in enumerate(body):
        if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", line):
            inside = line.startswith(".L" + head + ":") or ("Header=" + head + " ") in line + " " or ("Parent Loop " + head + " ") in line + " "
        if inside:
            out.append(line)
    return out


def count(region):
    c = collections.Counter()
    for line in region:
        m = re.match(r"^\s+([a-z]\w+)", line)
        if not m:
            continue
        op = m.group(1)
        for col, pat in COLUMNS:
            if re.match(pat, op):
                c[col] += 1
    return c


def resources(path, keys):
    """the compiler's resource comments behind every kernel: NumVgprs, TotalNumSgprs, ScratchSize, LDSByteSize"""
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1) if any(k in m.group(1) for k in keys) else None
            continue
        if name:
            m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|LDSByteSize): (\d+)", line)
            if m:
                out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm", nargs="?")
    ap.add_argument("--kernels", nargs="+", default=["k_wpair8ILi2", "k_pair8ILi0ELi12ELi0ELb1", "k_pair8ILi0ELi8ELi0ELb1", "k_pair8ILi0ELi4ELi0ELb1"])
    a = ap.parse_args()
    path = a.asm
    if not path:
        import isa_hazards
        path = isa_hazards.compile_to_asm()
    res = resources(path, a.kernels)
    cols = [c for c, _ in COLUMNS]
    print("| kernel | loop | VGPR | SGPR | LDS | scratch | " + " | ".join(cols) + " |")
    print("|" + "---|" * (6 + len(cols)))
    for name, body in sorted(functions(path, a.kernels)):
        r = res.get(name, {})
        for k, (lo, hi) in enumerate(march_loops(body)):
            c = count(loop_blocks(body, lo))
            print(f"| {name} | {k} | {r.get('NumVgprs')} | {r.get('TotalNumSgprs')} | {r.get('LDSByteSize')} | "
                  f"{r.get('ScratchSize')} | " + " | ".join(str(c[x]) for x in cols) + " |")


if __name__ == "__main__":
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    main()
