"""Block matching without a GPU:
 * the restatement of the search (tests/block_match_ref.py) against an independent brute-force statement in exact rationals, and the
   cases of tests/block_match_cases.py showing on the restatement what each is there for;
 * f3d_block_match_solve: the program tests/block_match_solve_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, and the
   host library through the package, against the restatement byte for byte, every branch of the rule among the cases;
 * the driver and the command-line tool on the host-memory stand-in of tests/cpu_device_block_match, the cases the GPU runs
   (tests/block_match_cases.py), and that stand-in's entries against the restatements;
 * the weak link: the host library on a device library without the two entries loads, solves, and the new calls name what is missing;
 * the command-line tool's refusals, each with exit 64 before any device is touched;
 * the new header: its entries are exported, have a wide-container case (the check tests/test_wide_container_coverage_cpu.py makes of
   include/f3d.h), and the layouts the package declares are the header's;
 * the quality case on the oracle's pyramid: the solve from the block-match guess ends below the cold solve and the hand guess."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import block_match_cases as cases
import block_match_ref as bm
import outlier_ref
import test_wide_container_coverage_cpu as coverage
import warm_start_ref as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "f3d_block_match.h")


def test_the_restatement_against_brute_force_in_exact_rationals():
    # integers on a range whose float32 arithmetic is exact: lo 0, hi 64, 64 bins -> the code is floor(s), 64 -> 63
    rng = np.random.default_rng(3)
    dims = (11, 9, 8)
    a = rng.integers(-3, 68, size=dims[::-1]).astype(np.float32)
    b = cases.rolled(a, (1, -1, 0))
    b[rng.random(b.shape) < 0.1] += 1.0
    a[1, 2, 3] = np.nan
    a[3:6, 3:6, 0:3] = 5.0           # node 0: flat
    b[:, :, 6:] = 9.0                # the last node sees a constant b wherever it looks: none
    grid = bm.Grid((1, 4, 4), 4, (3, 1, 1), 1, (1, 2, 1))
    records, info = bm.block_match(a, b, 0.0, 64.0, 64, grid)
    brute = bm.brute_force(a, b, 0.0, 64.0, 64, grid)
    assert [s for _, s in brute] == [bm.FLAT, bm.OK, bm.NONE] == list(records[:, 3])
    assert tuple(records[1, :3]) == brute[1][0] == (1, -1, 0)
    assert info["nodes"] == 3 and info["flat_nodes"] == info["none_nodes"] == 1 and info["nan"] == 0 and info["outside"] > 0
    # a tie: b == a with period 2 along x
    z, y, x = np.meshgrid(np.arange(7), np.arange(7), np.arange(12), indexing="ij")
    a = (10.0 * (x % 2) + 3.0 * y + z).astype(np.float32)
    grid = bm.Grid((5, 3, 3), 1, (2, 1, 1), 1, (2, 0, 0))
    records, _ = bm.block_match(a, a, 0.0, 64.0, 64, grid)
    brute = bm.brute_force(a, a, 0.0, 64.0, 64, grid)
    assert [tuple(r[:3]) for r in records] == [s for s, _ in brute] == [(-2, 0, 0)] * 2


def test_every_kernel_case_shows_what_it_is_there_for():
    seen = {}
    for case in cases.kernel_cases():
        records, info = case.expected()
        seen[case.name] = (records, info)
        assert records.shape == (case.grid.nodes, bm.RECORD_WORDS) and info["nodes"] == info["ok"] + info["flat_nodes"] + info["none_nodes"]
        total = np.prod([2 * r + 1 for r in case.grid.radii])
        searched = records[:, 3] != bm.FLAT
        assert (records[searched, 4:7].sum(axis=1) == total).all() and (records[~searched, 4:7] == 0).all()
    for name in ("w63", "w64", "w65"):
        assert seen[name][1]["outside"] > 0 and seen[name][1]["ok"] == seen[name][1]["nodes"] > 30
        assert 0 < (seen[name][0][:, 30] != 63).sum()                     # best shifts with a neighbour that is not valid
    assert seen["limit"][1]["evaluated"] == 17 ** 3 and tuple(seen["limit"][0][0, :3]) == (-7, 8, 5)
    assert tuple(seen["r4"][0][0, :3]) == (-3, 2, 4)
    flat = seen["flat"]
    assert flat[0][0, 3] == bm.FLAT and flat[1]["none_nodes"] >= 1 and flat[1]["flat"] > 0 and flat[1]["ok"] >= 2
    assert seen["nan"][1]["nan"] > 20
    assert seen["bins2"][0][:, 8].max() <= 125 and seen["bins2"][1]["ok"] > 0       # codes 0 and 1 only: saa <= n
    ties = seen["ties"][0]
    assert (ties[:, 3] == bm.OK).all() and (ties[:, 0] == -4).all() and (ties[:, 1] == -3).all() and (ties[:, 2] == -1).all()
    centre = seen["centre"]
    assert centre[0][0, 3] == bm.NONE and centre[0][0, 5] == 27
    hit = [i for i, r in enumerate(centre[0]) if r[3] == bm.OK and tuple(r[:3]) == (7, -6, 5)]
    assert len(hit) > 10


def test_the_recovery_case_on_the_restatement():
    case = cases.recovery_case()
    records, _ = case.expected()
    rows, summary = bm.solve(records, case.grid)
    cases.check_recovery(rows, case.grid)
    assert summary["low"] == 0
    # without the symmetry the shift and the ZNCC are as exact; the offsets are small, not 0
    case = cases.recovery_case(mirrored=False)
    rows, summary = bm.solve(case.expected()[0], case.grid)
    cases.check_recovery(rows, case.grid, offsets=False)
    assert summary["low"] == 0


def test_the_restatement_of_the_expansion_against_a_loop_over_the_voxels():
    f32 = np.float32
    for name, dims, _, origin, step, nodes in cases.expand_cases():
        if name.startswith("w6"):
            dims = (9, 5, 4)
        got = bm.expand_nodes(*nodes, origin, step, dims)
        nz, ny, nx = nodes[0].shape

        def axis(x, o, count):
            t = (f32(x) - f32(o)) / f32(step)
            i = min(max(int(np.floor(t)), 0), max(count - 2, 0))
            return i, min(max(t - f32(i), f32(0)), f32(1))

        def lerp(p, q, f):
            return f32(p + f32(f * f32(q - p)))

        with np.errstate(invalid="ignore"):
            for f, g in zip(nodes, got):
                for z in range(dims[2]):
                    for y in range(dims[1]):
                        for x in range(dims[0]):
                            (i, fx), (j, fy), (k, fz) = axis(x, origin[0], nx), axis(y, origin[1], ny), axis(z, origin[2], nz)
                            along_x = lambda jj, kk: lerp(f[kk, jj, i], f[kk, jj, i + 1], fx) if nx > 1 else f[kk, jj, 0]
                            along_y = lambda kk: lerp(along_x(j, kk), along_x(j + 1, kk), fy) if ny > 1 else along_x(0, kk)
                            want = lerp(along_y(k), along_y(k + 1), fz) if nz > 1 else along_y(0)
                            assert f32(want).tobytes() == g[z, y, x].tobytes() or (np.isnan(want) and np.isnan(g[z, y, x])), (name, x, y, z)
    # held constant outside the hull, NaN only where the NaN node takes part
    name, dims, _, origin, step, nodes = [c for c in cases.expand_cases() if c[0] == "hull_inside"][0]
    u = bm.expand_nodes(*nodes, origin, step, dims)[0]
    assert (u[:, :, :origin[0]] == u[:, :, origin[0]:origin[0] + 1]).all() and (u[:, :, -1] == u[:, :, origin[0] + 2 * step]).all()
    name, dims, _, origin, step, nodes = [c for c in cases.expand_cases() if c[0] == "nan_node"][0]
    u, v, w = bm.expand_nodes(*nodes, origin, step, dims)
    assert 0 < np.isnan(u).sum() < u.size and not np.isnan(v).any() and 0 < np.isnan(w).sum() < w.size


# ---- the host solve ---------------------------------------------------------------------------------------------------------------

def solve_cases():
    """(name, grid, records, centre, min_zncc): records of real searches, and drawn ones that reach every branch of the rule"""
    out = []
    for case in cases.kernel_cases():
        if case.name in ("w63", "flat", "nan", "ties", "centre", "bins2"):
            out.append((case.name, case.grid, case.expected()[0], case.centre, 0.5))
    case = cases.recovery_case()
    out.append(("recovery", case.grid, case.expected()[0], None, 0.5))
    rng = np.random.default_rng(17)
    grid = bm.Grid((4, 5, 6), 3, (10, 8, 6), 1, (2, 0, 3))
    records = np.zeros((grid.nodes, bm.RECORD_WORDS), np.int32)
    centre = rng.integers(-5, 6, (grid.nodes, 3)).astype(np.int32)
    for rec, c in zip(records, centre):
        win = rng.integers(0, 256, 27)
        rec[7], rec[8] = win.sum(), (win * win).sum()
        rec[3] = rng.choice([bm.OK] * 8 + [bm.FLAT, bm.NONE])
        rec[4:7] = rng.integers(0, 36, 3)
        if rec[3] != bm.OK:
            continue
        rec[0:3] = c + [rng.integers(-2, 3), 0, rng.integers(-3, 4)]
        for slot in range(7):     # the best shift and its six neighbours: windows near the one of a, some nearer than the best
            t = np.clip(win + rng.integers(-40, 41, 27) * rng.integers(0, 3), 0, 255)
            rec[9 + 3 * slot:12 + 3 * slot] = t.sum(), (t * t).sum(), (win * t).sum()
        rec[30] = rng.choice([63, 63, 63, rng.integers(0, 64)])
    out.append(("drawn", grid, records, centre, 0.6))
    return out


def branches(rows, records, grid, min_zncc):
    """which branches of the rule a set of rows went through"""
    n = (2 * grid.window + 1) ** 3
    seen = set(bm_status for bm_status in rows["status"])
    for r, row in zip(records, rows):
        if r[3] != bm.OK:
            continue
        da = n * int(r[8]) - int(r[7]) ** 2
        z0 = bm.zncc_of(n, int(r[7]), da, r[9:12])
        for axis in range(3):
            if (int(r[30]) >> (2 * axis)) & 3 != 3:
                seen.add("invalid neighbour")
                assert row["offset"][axis] == 0.0
                continue
            zm, zp = bm.zncc_of(n, int(r[7]), da, r[12 + 6 * axis:15 + 6 * axis]), bm.zncc_of(n, int(r[7]), da, r[15 + 6 * axis:18 + 6 * axis])
            if (zm - 2.0 * z0) + zp >= 0.0:
                seen.add("no peak")
                assert row["offset"][axis] == 0.0
            elif abs(row["offset"][axis]) == 0.5:
                seen.add("clamped")
            else:
                seen.add("parabola")
    return seen


@pytest.fixture(scope="module")
def solve_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("block_match_solve") / "block_match_solve_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cuda-flow3d_amd", "host"),
                    os.path.join(ROOT, "tests", "block_match_solve_main.cpp"), "-o", exe], check=True)
    return exe


def run_program(exe, tmp_path, grid_words, records, centre, min_zncc):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<12i", *grid_words, 0 if centre is None else 1))
        f.write(struct.pack("<d", min_zncc))
        f.write(np.ascontiguousarray(records, np.int32).tobytes())
        if centre is not None:
            f.write(np.ascontiguousarray(centre, np.int32).tobytes())
    if os.path.exists(dst):
        os.remove(dst)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return run, dst


def grid_words(grid):
    return [*grid.counts, *grid.origin, grid.step, grid.window, *grid.radii]


def test_the_host_solve_under_asan_and_ubsan_equals_the_restatement(solve_program, tmp_path):
    seen = set()
    for name, grid, records, centre, min_zncc in solve_cases():
        rows, summary = bm.solve(records, grid, centre, min_zncc)
        seen |= branches(rows, records, grid, min_zncc)
        run, dst = run_program(solve_program, tmp_path, grid_words(grid), records, centre, min_zncc)
        assert run.returncode == 0 and run.stdout.strip() == "ok", (name, run.returncode, run.stdout[-500:], run.stderr[-3000:])
        blob = open(dst, "rb").read()
        assert len(blob) == 88 * grid.nodes + 48
        assert blob[:88 * grid.nodes] == rows.tobytes(), name
        assert struct.unpack("<6Q", blob[88 * grid.nodes:]) == tuple(summary[k] for k in ("nodes", "ok", "flat", "none", "low", "edge")), name
    assert seen == {bm.NODE_OK, bm.NODE_FLAT, bm.NODE_NONE, bm.NODE_LOW, bm.NODE_EDGE, "invalid neighbour", "no peak", "clamped", "parabola"}


def test_the_host_solve_refuses_under_asan_and_ubsan(solve_program, tmp_path):
    grid = bm.Grid((4, 5, 6), 3, (2, 1, 1), 1, 1)
    records = np.zeros((2, bm.RECORD_WORDS), np.int32)
    good = grid_words(grid)
    bad = {"step": (6, 0), "nx": (0, 0), "ny": (1, -1), "window0": (7, 0), "window9": (7, 9), "radius": (9, -1)}
    for name, (at, value) in bad.items():
        words = list(good)
        words[at] = value
        run, dst = run_program(solve_program, tmp_path, words, records, None, 0.5)
        assert run.returncode == 3 and "f3d_block_match_solve" in run.stdout and not os.path.exists(dst), (name, run.stdout, run.stderr[-2000:])
    run, _ = run_program(solve_program, tmp_path, good, records, None, float("nan"))
    assert run.returncode == 3 and "NaN" in run.stdout
    run, _ = run_program(solve_program, tmp_path, good, records, None, 0.5)
    assert run.returncode == 0


def test_the_host_library_through_the_package_equals_the_restatement(f3d):
    for name, grid, records, centre, min_zncc in solve_cases():
        rows, summary = bm.solve(records, grid, centre, min_zncc)
        g = f3d.BlockMatchGrid(*grid.origin, grid.step, *grid.counts, grid.window, *grid.radii)
        got, got_summary = f3d.solve_block_match(records, g, centre, min_zncc)
        assert got.dtype == bm.NODE_DTYPE and got.tobytes() == rows.tobytes(), name
        assert got_summary == summary, name
    g = f3d.BlockMatchGrid(1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(f3d.F3dError, match="f3d_block_match_solve"):
        f3d.solve_block_match(np.zeros((1, 32), np.int32), g)
    with pytest.raises(ValueError):
        f3d.solve_block_match(np.zeros((2, 32), np.int32), f3d.BlockMatchGrid(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1))


# ---- the header -------------------------------------------------------------------------------------------------------------------

def test_every_entry_of_the_new_header_is_exported_and_has_a_wide_container_case(f3d):
    text = open(HEADER).read()
    entries = coverage.device_entries(text)
    assert entries == ["f3d_block_match", "f3d_expand_nodes"]
    assert [name for name, _ in coverage.declarations(text)] == entries
    assert [e for e in entries if not hasattr(f3d.hip(), e)] == []
    module = coverage.read("tests", "test_gpu_wide_container_block_match.py")
    assert coverage.uncovered(entries, [module], {}) == []
    assert coverage.uncovered(entries, [module.replace("f3d_expand_nodes", "f3d_e_n")], {}) == ["f3d_expand_nodes"]
    # f3d.h does not include the new header, and declares neither entry
    main = coverage.read("include", "f3d.h")
    assert "f3d_block_match" not in main and "f3d_expand_nodes" not in main
    assert '#include "f3d.h"' in text


def fields_of(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    out = []
    for kind, names in re.findall(r"(unsigned long long|double|float|int)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)((?:\[\d+\])*)", n)
            count = int(np.prod([int(d) for d in re.findall(r"\[(\d+)\]", m.group(2))] or [1]))
            out.append((m.group(1), kind, count))
    return out


def test_the_layouts_of_the_package_match_the_headers(f3d):
    text = open(HEADER).read()
    host = open(os.path.join(ROOT, "include", "f3d_host.h")).read()
    assert [(n, "int", 1) for n, _ in f3d.BlockMatchGrid._fields_] == fields_of(text, "f3d_block_match_grid")
    assert [(n, "unsigned long long", 1) for n, _ in f3d.BlockMatchInfo._fields_] == fields_of(text, "f3d_block_match_info")
    assert [(n, "unsigned long long", 1) for n, _ in f3d.BlockMatchSummary._fields_] == fields_of(host, "f3d_block_match_summary")
    record = fields_of(text, "f3d_block_match_record")
    assert all(kind == "int" for _, kind, _ in record) and sum(c for _, _, c in record) == f3d.BLOCK_MATCH_RECORD_WORDS == bm.RECORD_WORDS
    assert [n for n, _, _ in record] == ["shift", "status", "evaluated", "outside", "flat", "sa", "saa", "best", "neighbour", "valid", "nan"]
    kinds = {"int": np.int32, "double": np.float64, "float": np.float32}
    node = fields_of(host, "f3d_block_match_node")
    assert [(n, np.dtype(kinds[k]), c) for n, k, c in node] == \
        [(n, f3d.BLOCK_MATCH_NODE[n].base, int(np.prod(f3d.BLOCK_MATCH_NODE[n].shape or (1,)))) for n in f3d.BLOCK_MATCH_NODE.names]
    assert f3d.BLOCK_MATCH_NODE == bm.NODE_DTYPE and f3d.BLOCK_MATCH_NODE.itemsize == 88
    for name, value in (("OK", bm.NODE_OK), ("FLAT", bm.NODE_FLAT), ("NONE", bm.NODE_NONE), ("LOW", bm.NODE_LOW), ("EDGE", bm.NODE_EDGE)):
        assert re.search(r"#define F3D_BLOCK_NODE_%s %d\b" % (name, value), host)
        assert f3d.BLOCK_NODE_STATUS[value] == name.lower()


def test_the_grid_of_the_package_and_its_refusals(f3d):
    g = f3d.block_match_grid((48, 40, 24), **cases.QUALITY)
    ref = cases.default_grid((48, 40, 24), 6, 3, 7)
    assert (g.ox, g.oy, g.oz, g.step, g.nx, g.ny, g.nz, g.window, g.rx, g.ry, g.rz) == (*ref.origin, 6, *ref.counts, 3, 7, 7, 7)
    g = f3d.block_match_grid((512, 512, 512))
    assert (g.ox, g.nx, g.step, g.window, g.rx) == (15, 31, 16, 8, 8) and g.ox + 30 * 16 + 8 <= 511
    g = f3d.block_match_grid((40, 30, 20), step=5, window=2, search=(3, 0, 2), origin=(4, 2, 2), counts=(3, 1, 2))
    assert (g.ox, g.oy, g.oz, g.nx, g.ny, g.nz, g.rx, g.ry, g.rz) == (4, 2, 2, 3, 1, 2, 3, 0, 2)
    for bad in (dict(dims=(16, 40, 40)), dict(dims=(40, 40, 40), origin=(7, 8, 8)), dict(dims=(40, 40, 40), counts=(3, 1, 1)),
                dict(dims=(40, 40, 40), step=0), dict(dims=(40, 40, 40), search=(1, 2))):
        with pytest.raises(ValueError):
            f3d.block_match_grid(**bad)


# ---- the command-line tool: every refusal exits with 64 and the usage before any device is touched ---------------------------------

EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
REFUSALS = {
    "initial-flow": (2, ["--block-match", "--block-match-window", "2", "--initial-flow", "U", "V", "W"], "choose one"),
    "partial": (2, ["--block-match", "--block-match-window", "2", "--partial"], "--partial"),
    "concurrent": (3, ["--block-match", "--block-match-window", "2", "--concurrent", "2"], "--concurrent"),
    "warm-start": (3, ["--block-match", "--block-match-window", "2", "--warm-start"], "--warm-start"),
    "total": (3, ["--block-match", "--block-match-window", "2", "--total"], "--total"),
    "only-sequence": (3, ["--block-match", "--block-match-window", "2", "--block-match-only"], "one pair"),
    "window-leaves": (2, ["--block-match"], "leaves the volume"),
    "window-leaves-7": (2, ["--block-match", "--block-match-window", "6"], "leaves the volume"),
    "reach": (2, ["--block-match", "--block-match-window", "2", "--block-match-search", "15"], "at most 16"),
    "window-9": (2, ["--block-match", "--block-match-window", "9"], "usage:"),
    "window-0": (2, ["--block-match", "--block-match-window", "0"], "usage:"),
    "step-0": (2, ["--block-match", "--block-match-step", "0"], "usage:"),
    "search-two": (2, ["--block-match", "--block-match-search", "3:4"], "usage:"),
    "search-four": (2, ["--block-match", "--block-match-search", "1:2:3:4"], "usage:"),
    "search-negative": (2, ["--block-match", "--block-match-search", "-1"], "usage:"),
    "zncc-nan": (2, ["--block-match", "--block-match-min-zncc", "nan"], "usage:"),
    "option-alone": (2, ["--block-match-step", "4"], "need --block-match"),
    "only-alone": (2, ["--block-match-only"], "need --block-match"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_flow3d_refuses_before_any_device_is_touched(tmp_path, case):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    frames, extra, needle = REFUSALS[case]
    paths = []
    for i in range(frames):
        paths.append(str(tmp_path / f"f{i}.raw"))
        np.zeros((12, 12, 12), np.float32).tofile(paths[-1])
    files = {}
    for name in "UVW":
        files[name] = str(tmp_path / f"guess_{name}.raw")
        np.zeros((12, 12, 12), np.float32).tofile(files[name])
    extra = [files.get(a, a) for a in extra]
    run = subprocess.run([EXE, "--dims", "12", "12", "12", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage: flow3d" in run.stdout, run.stdout[-1500:]
    assert "--block-match [--block-match-step S]" in run.stdout


def test_the_layout_of_the_host_library_is_the_grid_of_the_package(f3d):
    for dims, step, window, radii in (((48, 40, 24), 6, 3, (7, 7, 7)), ((512, 512, 512), 16, 8, (8, 8, 8)), ((65, 20, 18), 5, 3, (2, 1, 2)),
                                      ((17, 17, 17), 1, 8, (0, 8, 3))):
        laid = f3d.BlockMatchGrid()
        assert f3d.host().f3d_block_match_layout(*dims, step, window, *radii, C.byref(laid)) == 0
        own = f3d.block_match_grid(dims, step, window, radii)
        assert [getattr(laid, n) for n, _ in laid._fields_] == [getattr(own, n) for n, _ in own._fields_]
    untouched = f3d.BlockMatchGrid(ox=77)
    for dims, step, window, radii in (((16, 40, 40), 16, 8, (8, 8, 8)), ((40, 40, 40), 0, 3, (1, 1, 1)), ((40, 40, 40), 4, 9, (1, 1, 1)),
                                      ((40, 40, 40), 4, 3, (1, -1, 1)), ((40, 40, 40), 4, 3, (1, 14, 1)), ((400, 400, 400), 1, 3, (1, 1, 1))):
        assert f3d.host().f3d_block_match_layout(*dims, step, window, *radii, C.byref(untouched)) != 0
        assert b"block matching" in f3d.host().f3d_host_last_error() and untouched.ox == 77
    assert f3d.host().f3d_block_match_layout(40, 40, 40, 4, 3, 1, 1, 1, None) != 0


# ---- the weak link: the host library loads against a device library without the two entries, and the calls name them -------------

WEAK = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in, which has neither entry
    W, H, D = 26, 22, 20
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=3, outer_iterations_count=2)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    plain = flow.compute(f0, f1, silent=True, **kw)       # the host library loads and solves without the entries
    flow.upload(f0, f1)
    nodes = np.zeros((2, 2, 2), np.float32)
    calls = [(lambda: pkg.block_match(f0, f1, window=3), "f3d_block_match"), (lambda: flow.block_match(window=3), "f3d_block_match"),
             (lambda: pkg.expand_nodes(nodes, nodes, nodes, (3, 3, 3), 8, (W, H, D)), "f3d_expand_nodes"),
             (lambda: flow.compute_resident(silent=True, initial="block-match", **kw), "f3d_block_match"),
             (lambda: flow.set_initial_from_nodes(), "f3d_")]
    for call, name in calls:
        try:
            call(); raise SystemExit("a call succeeded without " + name)
        except pkg.F3dError as e:
            assert name in str(e), str(e)
    # what needs no device still works
    grid = pkg.block_match_grid((W, H, D), step=8, window=3, search=2)
    rows, summary = pkg.solve_block_match(np.zeros((grid.nx * grid.ny * grid.nz, 32), np.int32), grid)
    assert summary["nodes"] == len(rows) == grid.nx * grid.ny * grid.nz
    again = flow.compute(f0, f1, silent=True, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    flow.destroy()
    pkg.shutdown()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_entries_and_the_calls_name_them():
    cpu = os.path.join(ROOT, "tests", "cpu_device")
    subprocess.run(["make", "-C", cpu, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(cpu, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_block_match" not in names and "f3d_expand_nodes" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", WEAK], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- the driver and the command-line tool on the host-memory stand-in of tests/cpu_device_block_match ---------------------------------

STAND_IN = textwrap.dedent('''
    import importlib, os, sys
    sys.path.insert(0, os.environ["F3D_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["F3D_ROOT"], "tests"))
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in with the block matching entries
    import block_match_cases as cases
    what = sys.argv[1]
    assert all(hasattr(pkg.hip(), e) for e in ("f3d_block_match", "f3d_expand_nodes", "f3d_value_range", "f3d_validate_displacement"))
    if what == "entries":
        cases.check_entries(pkg)
    elif what == "driver":
        cases.check_driver(pkg)
    elif what == "cli":
        cases.check_cli(pkg, os.path.join(os.environ["F3D_TEST_LIBDIR"], "flow3d"), sys.argv[2])
    pkg.shutdown()
    print("ok", what)
''')


@pytest.fixture(scope="module")
def stand_in(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpu_device_block_match"))
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_device_block_match"), "OUT=" + out, "all", "-j4"], check=True,
                   stdout=subprocess.DEVNULL)
    return out


@pytest.mark.parametrize("what", ["entries", "driver", "cli"])
def test_the_driver_and_the_tool_on_the_cpu_backend(stand_in, tmp_path, what):
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=stand_in, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", STAND_IN, what, str(tmp_path)], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and f"ok {what}" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- quality, on the oracle's pyramid ---------------------------------------------------------------------------------------------

def test_a_solve_from_the_block_match_guess_ends_below_the_cold_solve_and_the_hand_guess(oracle):
    """Measured on the oracle: cold 3.303, from the hand guess (5, -3, 2) 0.505, from the block-match guess 0.069; the guess itself
    1.178 against the hand guess's 1.732.  The 8-bit windows of radius 3 lock on wherever the true shift is among a node's
    candidates (ZNCC 1.000); the nodes whose target window would leave the box pick a wrong shift with a high ZNCC, and the median
    test on the node grid replaces them."""
    f0, f1 = ws.test_pair()
    d, h, w = f0.shape
    grid = cases.default_grid((w, h, d), cases.QUALITY["step"], cases.QUALITY["window"], cases.QUALITY["search"])
    records, _ = bm.block_match(f0, f1, float(f0.min()), float(f0.max()), 256, grid)
    rows, _ = bm.solve(records, grid)
    nodes = [rows[k].reshape(grid.counts[::-1]) for k in "uvw"]
    _, u, v, ww, _ = outlier_ref.validate(*nodes)
    guess, _ = ws.initial_flow(*bm.expand_nodes(u, v, ww, grid.origin, grid.step, (w, h, d)))
    kw = dict(warp_levels_count=cases.QUALITY_LEVELS)
    cold = ws.pyramid(f0, f1, **kw)
    hand = ws.pyramid(f0, f1, initial=ws.initial_flow(*ws.constant_flow(f0.shape, ws.PAIR_GUESS))[0], **kw)
    matched = ws.pyramid(f0, f1, initial=guess, **kw)
    cases.check_quality(cold, hand, guess, matched)
