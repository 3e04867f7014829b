"""Subset correlation without a GPU: the numpy restatement of tests/subset_match_ref.py against the independent plain
statement beside it, the exact case, the analytic cases (relations, not numbers), every status among the cases of
tests/subset_match_cases.py, the host table and layout as a program of their own under ASan and UBSan and through the package byte
for byte, the header: its entry exported, the struct layouts the package's, the entry named in the wide-container module, and the
entry, the driver and the command-line tool on the host-memory stand-in of tests/cpu_device_subset_match."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import block_match_ref as bm
import subset_match_cases as cases
import subset_match_ref as sm
import test_wide_container_coverage_cpu as coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "f3d_subset_match.h")

# The restatement and the plain statement differ in the order of every sum and in how the Keys kernel, the normal equations and the
# composition are written.  Measured on the cases below: at most 5.3e-15 in a parameter between the two; times 10 for
# the summation order.
PLAIN_BOUND = 5.3e-14


def small_cases():
    """(name, a, b, grid, model, start, max_iterations): windows small enough for Python loops over the voxels"""
    dims = (22, 20, 18)
    a, b, truth = cases.analytic_pair(dims, cases.rotation_z(1.0) @ np.diag([1.01, 0.99, 1.0]), (0.3, -0.2, 0.25))
    grid = sm.Grid((6, 6, 6), 8, (2, 2, 1), 3)
    out = [("affine", a, b, grid, sm.AFFINE, None, 20), ("translation", a, b, grid, sm.TRANSLATION, None, 20),
           ("started", a, b, grid, sm.AFFINE, cases.starts_round(grid, truth, 0.3, 1), 20)]
    status = cases.status_case()
    few = sm.Grid(status.grid.origin, status.grid.step, (status.grid.counts[0], 2, 1), status.grid.window)
    out.append(("statuses", status.a, status.b, few, sm.AFFINE, status.start[:few.nodes], 6))
    return out


def test_the_restatement_against_the_plain_statement():
    worst, seen = 0.0, set()
    for name, a, b, grid, model, start, iterations in small_cases():
        records, _ = sm.subset_match(a, b, grid, model, start, iterations)
        for i, c in enumerate(grid.positions()):
            plain = sm.plain(a, b, c, grid.window, model, None if start is None else start[i], iterations)
            rec = records[i]
            assert plain["status"] == rec["status"] and plain["iterations"] == rec["iterations"], (name, i, plain, rec)
            seen.add(int(rec["status"]))
            if rec["status"] == sm.NO_START:
                continue
            worst = max(worst, float(np.abs(np.array(plain["p"]) - rec["p"]).max()))
            assert abs(plain["zncc"] - rec["zncc"]) <= 1e-12 and abs(plain["step"] - rec["step"]) <= PLAIN_BOUND * max(1, grid.window)
    print("restatement against the plain statement: at most %.3g in a parameter" % worst)
    assert worst <= PLAIN_BOUND
    assert {sm.OK, sm.NAN, sm.FLAT, sm.FLAT_TARGET, sm.OUTSIDE, sm.NO_START} <= seen


def test_the_result_is_stationary():
    """an OK node started again from its result takes one step, and that step is below the tolerance"""
    for name, a, b, grid, model, start, iterations in small_cases()[:3]:
        records, info = sm.subset_match(a, b, grid, model, start, iterations)
        ok = records["status"] == sm.OK
        assert ok.sum() >= 2, name
        again, _ = sm.subset_match(a, b, grid, model, records["p"], 1)
        assert (again["status"][ok] == sm.OK).all() and (again["step"][ok] < 1e-3).all(), (name, again["step"])


def test_the_exact_case_on_the_restatement():
    case = cases.exact_case()
    records, info = case.expected()
    cases.check_exact(records, case.start)
    assert info["status"][sm.OK] == case.grid.nodes == 18 and info["iterations"] == 18


@pytest.fixture(scope="module")
def strained():
    a, b, truth = cases.strained_pair()
    grid = cases.ANALYTIC_GRID
    return a, b, truth, grid, {m: sm.subset_match(a, b, grid, m)[0] for m in (sm.TRANSLATION, sm.AFFINE)}


def test_the_affine_model_is_closer_than_the_translation_model_under_strain(strained):
    a, b, truth, grid, records = strained
    assert all((r["status"] == sm.OK).all() for r in records.values())
    translation, affine = (cases.errors(records[m], grid, truth) for m in (sm.TRANSLATION, sm.AFFINE))
    print("1 %% strain + 1 degree: rms displacement error %.4f (translation) %.4f (affine); rms gradient error %.5f (affine)"
          % (translation[0], affine[0], affine[1]))
    assert affine[0] < translation[0]                       # (i)
    assert affine[1] < cases.STRAIN                          # (iii)


def test_a_sub_voxel_translation_is_found_by_both_models():
    a, b, truth = cases.translated_pair()
    for model in (sm.TRANSLATION, sm.AFFINE):
        records, info = sm.subset_match(a, b, cases.ANALYTIC_GRID, model)
        error = cases.errors(records, cases.ANALYTIC_GRID, truth)
        print("sub-voxel translation, model %d: rms displacement error %.4f, gradient %.5f" % (model, *error))
        assert info["status"][sm.OK] == cases.ANALYTIC_GRID.nodes
        # the start (zero) is 0.51 voxel from the truth; what is left is the bias of the cubic interpolation
        assert error[0] < 0.05 and (records["zncc"] > 0.999).all()


def test_the_result_from_the_block_match_start_is_closer_to_the_truth_than_that_start():
    """(ii): a motion block matching has to find, (2.37, -1.71, 1.29) voxels, then its shift + offset as the start"""
    a, b, truth = cases.translated_pair((2.37, -1.71, 1.29))
    grid = cases.ANALYTIC_GRID
    records, _ = bm.block_match(a, b, float(a.min()), float(a.max()), 256, bm.Grid(grid.origin, grid.step, grid.counts, grid.window, 3))
    rows, summary = bm.solve(records, bm.Grid(grid.origin, grid.step, grid.counts, grid.window, 3), None, 0.5)
    assert summary["ok"] == grid.nodes
    start = np.zeros((grid.nodes, 12))
    for k, name in enumerate("uvw"):
        start[:, 4 * k] = rows[name]
    want = np.array([truth(c) for c in grid.positions()])
    before = np.sqrt(((start - want)[:, 0::4] ** 2).sum(axis=1))
    refined, info = sm.subset_match(a, b, grid, sm.AFFINE, start)
    after = np.sqrt(((refined["p"] - want)[:, 0::4] ** 2).sum(axis=1))
    print("block-match start: rms error %.4f, refined %.4f" % (np.sqrt((before ** 2).mean()), np.sqrt((after ** 2).mean())))
    assert info["status"][sm.OK] == grid.nodes
    assert (after < before).all()


def test_every_kernel_case_shows_what_it_is_there_for():
    by_name = {c.name: c for c in cases.kernel_cases()}
    seen = set()
    for c in by_name.values():
        seen |= c.statuses()
        assert c.expected()[1]["nodes"] == c.grid.nodes and sum(c.expected()[1]["status"]) == c.grid.nodes
    assert seen == set(range(9)), "a status is missing among the cases"
    status = by_name["statuses"].expected()[0]["status"]
    assert {i: int(status[i]) for i in cases.STATUS_NODES} == cases.STATUS_NODES
    assert by_name["statuses"].expected()[0]["nan"][0] == 1 and by_name["statuses"].expected()[0]["nan"][1] == 0
    assert by_name["singular"].statuses() == {sm.SINGULAR}
    lost = by_name["lost"].expected()[0]
    assert lost["status"][0] == sm.OK and (lost["status"][1:] == sm.LOST).all()
    one = by_name["one_iteration"].expected()[0]
    assert (one["status"] == sm.NOT_CONVERGED).all() and (one["iterations"] == 1).all()
    assert (by_name["64_iterations"].expected()[0]["iterations"] == 64).all()
    # the faces: every node has a tap on voxel 0 or on the last voxel of each axis and is inside; a hair further it is outside
    faces = by_name["faces"]
    assert sm.OUTSIDE not in faces.statuses() and (faces.expected()[0]["iterations"] == 1).all()
    n, W = faces.dims[0], faces.grid.window
    assert {c - W - 1 for c in (2, n - 4)} == {0, n - 6} and {c + W + 2 for c in (2, n - 4)} == {5, n - 1}
    beyond = by_name["beyond_faces"].expected()[0]["status"]
    assert [i for i in range(8) if beyond[i] == sm.OUTSIDE] == [0, 1, 2, 4, 7]
    assert {c.dims[0] for c in by_name.values()} >= {63, 64, 65}
    assert {c.grid.window for c in by_name.values()} >= {1, 2, 3, 8} and {c.model for c in by_name.values()} == {sm.TRANSLATION, sm.AFFINE}
    assert by_name["W8"].grid.nodes == 8 and all(c.a.size <= 41 * 36 * 33 for c in by_name.values())
    far = by_name["far_start"]
    assert far.statuses() == {sm.OK} and abs(far.expected()[0]["p"][0, 0] - 23.0) < 0.1


# ---- the host table and layout -----------------------------------------------------------------------------------------------------

def table_cases():
    """(name, grid, records, min_zncc, compare)"""
    status = cases.status_case()
    records = status.expected()[0]
    n = status.grid.nodes
    compare = [np.random.default_rng(k).normal(0.3, 0.2, n).astype(np.float32) for k in range(3)]
    compare[1][7] = np.nan
    out = [("statuses", status.grid, records, 0.9, compare), ("no compare", status.grid, records, 0.9, None),
           ("all low", status.grid, records, 2.0, compare), ("none low", status.grid, records, -1.0, compare)]
    one = sm.Grid((3, 3, 3), 1, (1, 1, 1), 1)
    out.append(("one node", one, records[6:7], 0.5, [c[:1] for c in compare]))
    for name in ("singular", "lost"):
        c = [c for c in cases.kernel_cases() if c.name == name][0]
        out.append((name, c.grid, c.expected()[0], 0.8, [np.zeros(c.grid.nodes, np.float32)] * 3))
    return out


@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subset_match_table") / "subset_match_table_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cuda-flow3d_amd", "host"),
                    os.path.join(ROOT, "tests", "subset_match_table_main.cpp"), "-o", exe], check=True)
    return exe


def grid_words(grid):
    return [*grid.origin, grid.step, *grid.counts, grid.window]


def run_table(exe, tmp_path, words, records, min_zncc, compare):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<10i", *words, 0 if compare is None else 1, 0))
        f.write(struct.pack("<d", min_zncc))
        f.write(np.ascontiguousarray(records).tobytes())
        for c in compare or []:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
    if os.path.exists(dst):
        os.remove(dst)
    run = subprocess.run([exe, "table", src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return run, dst


def summary_of(blob):
    words = struct.unpack("<12Q4d", blob)
    return dict(nodes=words[0], status=list(words[1:11]), compared=words[11], median_zncc=words[12], rms=words[13], median=words[14],
                p95=words[15])


def same(got, want):
    assert sorted(got) == sorted(want)
    return all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() if isinstance(want[k], float) else got[k] == want[k] for k in want)


def test_the_host_table_under_asan_and_ubsan_equals_the_restatement(table_program, tmp_path):
    seen = set()
    for name, grid, records, min_zncc, compare in table_cases():
        rows, summary = sm.table(records, grid, min_zncc, compare)
        seen |= set(int(s) for s in rows["status"])
        run, dst = run_table(table_program, tmp_path, grid_words(grid), records, min_zncc, compare)
        assert run.returncode == 0 and run.stdout.strip() == "ok", (name, run.returncode, run.stdout[-500:], run.stderr[-3000:])
        blob = open(dst, "rb").read()
        assert len(blob) == 96 * grid.nodes + 128
        assert blob[:96 * grid.nodes] == rows.tobytes(), name
        assert same(summary_of(blob[96 * grid.nodes:]), summary), (name, summary_of(blob[96 * grid.nodes:]), summary)
        assert sum(summary["status"]) == grid.nodes
    assert seen == set(range(10)), "a status of the table is missing among its cases"
    _, grid, records, min_zncc, compare = table_cases()[0]
    rows, summary = sm.table(records, grid, min_zncc, compare)
    assert summary["compared"] > 2 and summary["rms"] >= summary["median"] > 0 and summary["p95"] >= summary["median"]
    assert sm.table(records, grid, 2.0, compare)[1]["status"][sm.LOW] > 0 and np.isnan(rows["u"][rows["status"] != sm.OK]).all() and np.isnan(rows["diff"][7][1])


def test_the_host_table_and_layout_refuse_under_asan_and_ubsan(table_program, tmp_path):
    grid = sm.Grid((4, 5, 6), 3, (2, 1, 1), 1)
    records = np.zeros(2, sm.RECORD)
    good = grid_words(grid)
    for name, (at, value) in {"step": (3, 0), "nx": (4, 0), "ny": (5, -1), "window0": (7, 0), "window9": (7, 9), "below": (1, -3),
                              "beyond": (2, 2 ** 31 - 2), "far step": (3, 2 ** 30 + 1)}.items():
        words = list(good)
        words[at] = value
        run, dst = run_table(table_program, tmp_path, words, records, 0.5, None)
        assert run.returncode == 3 and "f3d_subset_match_table" in run.stdout and not os.path.exists(dst), (name, run.stdout, run.stderr[-2000:])
    run, _ = run_table(table_program, tmp_path, good, records, float("nan"), None)
    assert run.returncode == 3 and "NaN" in run.stdout
    assert run_table(table_program, tmp_path, good, records, 0.5, None)[0].returncode == 0
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for dims, step, window in (((40, 36, 33), 8, 2), ((19, 19, 19), 16, 8), ((64, 21, 30), 5, 3), ((100, 7, 9), 1, 2)):
        run = subprocess.run([table_program, "layout", *map(str, dims), str(step), str(window)], capture_output=True, text=True, env=env)
        assert run.returncode == 0 and [int(x) for x in run.stdout.split()] == grid_words(sm.default_grid(dims, step, window)), run.stdout
    for dims, step, window in (((18, 19, 19), 16, 8), ((40, 40, 6), 4, 2), ((40, 40, 40), 0, 2), ((40, 40, 40), 4, 9), ((40, 40, 40), 4, 0),
                               ((400, 400, 400), 1, 1)):
        run = subprocess.run([table_program, "layout", *map(str, dims), str(step), str(window)], capture_output=True, text=True, env=env)
        assert run.returncode == 3 and "subset correlation" in run.stdout, (dims, step, window, run.stdout, run.stderr[-2000:])


def test_the_host_library_through_the_package_equals_the_restatement(f3d):
    for name, grid, records, min_zncc, compare in table_cases():
        rows, summary = sm.table(records, grid, min_zncc, compare)
        got, got_summary = f3d.subset_table(records, f3d.SubsetGrid(*grid_words(grid)), min_zncc, compare)
        assert got.dtype == sm.ROW and got.tobytes() == rows.tobytes(), name
        assert same(got_summary, summary), name
    with pytest.raises(f3d.F3dError, match="f3d_subset_match_table"):
        f3d.subset_table(np.zeros(1, sm.RECORD), f3d.SubsetGrid(1, 1, 1, 0, 1, 1, 1, 1))
    with pytest.raises(ValueError):
        f3d.subset_table(np.zeros(2, sm.RECORD), f3d.SubsetGrid(1, 1, 1, 1, 1, 1, 1, 1))
    # positions that would not fit an int are refused, not computed
    for bad in (f3d.SubsetGrid(-1, 1, 1, 1, 1, 1, 1, 1), f3d.SubsetGrid(1, 1, 2 ** 31 - 5, 1, 1, 1, 1, 1),
                f3d.SubsetGrid(1, 1, 1, 2 ** 30, 1, 3, 1, 1)):
        rows = 3 if bad.ny == 3 else 1
        with pytest.raises(f3d.F3dError, match="2\\^30"):
            f3d.subset_table(np.zeros(rows, sm.RECORD), bad)
    for dims, step, window in (((40, 36, 33), 8, 2), ((19, 19, 19), 16, 8), ((64, 21, 30), 5, 3)):
        laid = f3d.SubsetGrid()
        assert f3d.host().f3d_subset_match_layout(*dims, step, window, C.byref(laid)) == 0
        want = grid_words(sm.default_grid(dims, step, window))
        assert [getattr(laid, n) for n, _ in laid._fields_] == want
        assert [getattr(f3d.subset_grid(dims, step, window), n) for n, _ in laid._fields_] == want
    assert f3d.host().f3d_subset_match_layout(18, 40, 40, 16, 8, C.byref(laid)) != 0 and b"subset correlation" in f3d.host().f3d_host_last_error()
    assert f3d.host().f3d_subset_match_layout(40, 40, 40, 4, 3, None) != 0


# ---- the header -------------------------------------------------------------------------------------------------------------------

def test_the_entry_of_the_new_header_is_exported_and_has_a_wide_container_case(f3d):
    text = open(HEADER).read()
    entries = coverage.device_entries(text)
    assert entries == ["f3d_subset_match"]
    assert [name for name, _ in coverage.declarations(text)] == entries
    assert hasattr(f3d.hip(), "f3d_subset_match")
    module = coverage.read("tests", "test_gpu_wide_container_subset_match.py")
    assert coverage.uncovered(entries, [module], {}) == []
    assert coverage.uncovered(entries, [module.replace("f3d_subset_match", "f3d_s_m")], {}) == ["f3d_subset_match"]
    # neither f3d.h nor f3d_block_match.h includes the new header or declares the entry
    for other in ("f3d.h", "f3d_block_match.h"):
        assert "f3d_subset_match" not in coverage.read("include", other)
    assert '#include "f3d.h"' in text


def fields_of(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    defines = dict(re.findall(r"#define (F3D_\w+) (\d+)", text))
    out = []
    for kind, names in re.findall(r"(unsigned long long|double|float|int)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)((?:\[\w+\])*)", n)
            count = int(np.prod([int(defines.get(d, d)) for d in re.findall(r"\[(\w+)\]", m.group(2))] or [1]))
            out.append((m.group(1), kind, count))
    return out


def test_the_layouts_of_the_package_match_the_headers(f3d, table_program):
    text = open(HEADER).read()
    host = open(os.path.join(ROOT, "include", "f3d_host.h")).read()
    kinds = {"int": np.int32, "double": np.float64, "float": np.float32}
    ckinds = {"int": C.c_int, "unsigned long long": C.c_ulonglong, "double": C.c_double}

    def of_dtype(dtype):
        return [(n, dtype[n].base, int(np.prod(dtype[n].shape or (1,)))) for n in dtype.names]

    def of_struct(cls):
        return [(n, t._type_, t._length_) if hasattr(t, "_length_") else (n, t, 1) for n, t in cls._fields_]

    assert [(n, np.dtype(kinds[k]), c) for n, k, c in fields_of(text, "f3d_subset_match_record")] == of_dtype(f3d.SUBSET_RECORD)
    assert [(n, np.dtype(kinds[k]), c) for n, k, c in fields_of(host, "f3d_subset_match_node")] == of_dtype(f3d.SUBSET_NODE)
    assert f3d.SUBSET_RECORD == sm.RECORD and f3d.SUBSET_NODE == sm.ROW
    assert [(n, ckinds[k], c) for n, k, c in fields_of(text, "f3d_subset_match_grid")] == of_struct(f3d.SubsetGrid)
    assert [(n, ckinds[k], c) for n, k, c in fields_of(text, "f3d_subset_match_info")] == of_struct(f3d.SubsetInfo)
    assert [(n, ckinds[k], c) for n, k, c in fields_of(host + text, "f3d_subset_match_summary")] == of_struct(f3d.SubsetSummary)
    # the compiler's sizes are the package's: no padding anywhere
    sizes = subprocess.run([table_program, "sizes"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert [int(x) for x in sizes.stdout.split()] == [144, 96, 128, C.sizeof(f3d.SubsetInfo), C.sizeof(f3d.SubsetGrid)] == [144, 96, 128, 96, 32]
    assert f3d.SUBSET_RECORD.itemsize == 144 and f3d.SUBSET_NODE.itemsize == 96 and C.sizeof(f3d.SubsetSummary) == 128
    assert [f3d.SUBSET_RECORD.fields[n][1] for n in ("p", "zncc", "step", "df", "dg", "status", "iterations", "nan")] == \
        [0, 96, 104, 112, 120, 128, 132, 136]
    for value, name in enumerate(sm.STATUS):
        where = host if name == "low" else text
        assert re.search(r"#define F3D_SUBSET_%s%s %d\b" % ("NODE_" if name == "low" else "", name.upper(), value), where), name
        assert f3d.SUBSET_STATUS[value] == name
    assert re.search(r"#define F3D_SUBSET_TRANSLATION 0\b", text) and re.search(r"#define F3D_SUBSET_AFFINE 1\b", text)
    assert f3d.SUBSET_MODELS == {"translation": sm.TRANSLATION, "affine": sm.AFFINE}
    assert re.search(r"#define F3D_SUBSET_MATCH_LANES %d\b" % sm.LANES, text)


def test_the_package_checks_its_arguments_without_a_device(f3d):
    with pytest.raises(ValueError):
        f3d.subset_grid((18, 40, 40))
    with pytest.raises(ValueError):
        f3d.subset_grid((40, 40, 40), step=0)
    with pytest.raises(ValueError):
        f3d.subset_grid((40, 40, 40), window=9)
    with pytest.raises(ValueError):
        f3d.subset_grid((40, 40, 40), window=3, origin=(3, 4, 4))
    g = f3d.subset_grid((40, 40, 40), step=8, window=3, origin=(6, 6, 6), counts=(2, 3, 4))
    assert (g.ox, g.step, g.nx, g.ny, g.nz, g.window) == (6, 8, 2, 3, 4, 3)
    assert f3d._subset_start(None, 5) is None and f3d._subset_start([np.ones(5)] * 3, 5)[:, 0::4].tolist() == [[1.0] * 3] * 5
    with pytest.raises(ValueError):
        f3d._subset_start(np.zeros(13), 1)
    # [nodes, 12] as a list for three nodes is not three node arrays
    listed = [[float(12 * n + k) for k in range(12)] for n in range(3)]
    assert f3d._subset_start(listed, 3).tolist() == listed
    assert f3d._subset_start([np.arange(3.0)] * 3, 3)[:, 4].tolist() == [0.0, 1.0, 2.0]


# ---- the weak link: the host library loads against a device library without the entry, and the calls name it ------------------------

WEAK = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in, which has no f3d_subset_match
    W, H, D = 26, 22, 20
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=3, outer_iterations_count=2)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    plain = flow.compute(f0, f1, silent=True, **kw)       # the host library loads and solves without the entry
    flow.upload(f0, f1)
    flow.compute_resident(silent=True, **kw)
    for call in (lambda: pkg.subset_match(f0, f1, grid=pkg.subset_grid((W, H, D), 8, 3)), lambda: flow.subset_match(start="zero", step=8, window=3),
                 lambda: flow.subset_match(start="flow", step=8, window=3)):
        try:
            call(); raise SystemExit("a call succeeded without f3d_subset_match")
        except pkg.F3dError as e:
            assert "f3d_subset_match" in str(e), str(e)
    # what needs no device still works
    grid = pkg.subset_grid((W, H, D), step=8, window=3)
    rows, summary = pkg.subset_table(np.zeros(grid.nx * grid.ny * grid.nz, pkg.SUBSET_RECORD), grid)
    assert summary["nodes"] == len(rows) == grid.nx * grid.ny * grid.nz
    again = flow.compute(f0, f1, silent=True, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    flow.destroy()
    pkg.shutdown()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_entry_and_the_calls_name_it():
    cpu = os.path.join(ROOT, "tests", "cpu_device")
    subprocess.run(["make", "-C", cpu, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(cpu, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_subset_match" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", WEAK], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- the entry, the driver and the command-line tool on the host-memory stand-in of tests/cpu_device_subset_match -----------------------

STAND_IN = textwrap.dedent('''
    import importlib, os, sys
    sys.path.insert(0, os.environ["F3D_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["F3D_ROOT"], "tests"))
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in with f3d_subset_match
    import subset_match_cases as cases
    what = sys.argv[1]
    assert hasattr(pkg.hip(), "f3d_subset_match") and hasattr(pkg.hip(), "f3d_block_match")
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
    out = str(tmp_path_factory.mktemp("cpu_device_subset_match"))
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_device_subset_match"), "OUT=" + out, "all", "-j4"], check=True,
                   stdout=subprocess.DEVNULL)
    return out


@pytest.mark.parametrize("what", ["entries", "driver", "cli"])
def test_the_entry_the_driver_and_the_tool_on_the_cpu_backend(stand_in, tmp_path, what):
    """entries: the stand-in's plain loops against the restatement bit for bit on every kernel case.  driver: SubsetMatch from each
    start source (the nearest-node mapping, the flow read at the nodes, the NaN of a node that is neither ok nor edge) against the
    same steps by hand.  cli: the CSV and the printed line of one pair and of a sequence against the Python calls."""
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=stand_in, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", STAND_IN, what, str(tmp_path)], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and f"ok {what}" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- flow3d --subset-match: every refusal exits with 64 before any device is touched --------------------------------------------------

EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
SUBSET = ["--subset-match", "--subset-window", "2"]
REFUSALS = {
    "partial": (2, SUBSET + ["--partial"], "--partial"),
    "concurrent": (3, SUBSET + ["--concurrent", "2"], "--concurrent"),
    "sequence-partial": (3, SUBSET + ["--partial"], "--partial"),
    "start-without-block-match": (2, SUBSET + ["--subset-start", "block-match"], "needs --block-match"),
    "start-with-only": (2, SUBSET + ["--subset-start", "block-match", "--block-match", "--block-match-window", "2", "--block-match-only"],
                        "needs --block-match"),
    "window-leaves": (2, ["--subset-match"], "leave the volume"),
    "window-leaves-5": (2, ["--subset-match", "--subset-window", "5"], "leave the volume"),
    "window-9": (2, ["--subset-match", "--subset-window", "9"], "usage:"),
    "window-0": (2, ["--subset-match", "--subset-window", "0"], "usage:"),
    "step-0": (2, SUBSET + ["--subset-step", "0"], "usage:"),
    "iterations-0": (2, SUBSET + ["--subset-iterations", "0"], "usage:"),
    "iterations-65": (2, SUBSET + ["--subset-iterations", "65"], "usage:"),
    "tolerance-0": (2, SUBSET + ["--subset-tolerance", "0"], "usage:"),
    "tolerance-nan": (2, SUBSET + ["--subset-tolerance", "nan"], "usage:"),
    "zncc-nan": (2, SUBSET + ["--subset-min-zncc", "nan"], "usage:"),
    "model": (2, SUBSET + ["--subset-model", "quadratic"], "usage:"),
    "start": (2, SUBSET + ["--subset-start", "guess"], "usage:"),
    "option-alone": (2, ["--subset-step", "4"], "need --subset-match"),
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
    run = subprocess.run([EXE, "--dims", "12", "12", "12", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage: flow3d" in run.stdout, run.stdout[-1500:]
    assert "--subset-match [--subset-step S]" in run.stdout
