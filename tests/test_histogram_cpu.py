"""The grey-value histogram and the Otsu thresholds without a GPU: the restatement (tests/histogram_ref.py) against independent forms
(an enumeration of every float32 of a narrow range with the product formed exactly in binary64, counts through the edges, exact
rational arithmetic for the objective), the host functions f3d_histogram_edge, f3d_otsu and f3d_histogram_rank against the restatement
bit for bit, the same functions in a stand-alone program under AddressSanitizer and UBSan, the struct layouts, the binding's argument
checks, the message of a device library without f3d_histogram, and the refusals of bin/flow3d.

The bound of the exact-arithmetic test is derived, not chosen: every term M * M / N of the objective takes two roundings and the sum of
two or three positive terms at most two more, so the computed objective lies within a factor (1 +- 2^-53)^4 < 1 +- 5 * 2^-53 of the
exact one; the chosen cut's computed objective is at least the computed objective of the exact argmax, hence its exact objective is
at least (1 - 5 * 2^-53)^2 > 1 - 2^-49 times the exact maximum."""
import ctypes as C
import functools
import os
import subprocess
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest

import histogram_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
NARROW = (F32(1), F32(1) + F32(2.0 ** -10))


@functools.lru_cache(maxsize=None)
def narrow_floats():
    """every float32 of [1, 1 + 2^-10]: 8193 values"""
    lo, hi = NARROW
    bits = np.arange(lo.view(np.uint32), hi.view(np.uint32) + 1, dtype=np.uint32)
    values = bits.view(F32)
    assert len(values) == 8193 and values[0] == lo and values[-1] == hi
    values.setflags(write=False)
    return values


def exact_bins(values, lo, hi, bins):
    """the bin rule one scalar at a time with the product formed in binary64, where it is exact (24 + 24 bits), and rounded once"""
    scale = ref.scale_of(lo, hi, bins)
    out = []
    for s in values:
        offset = F32(np.float64(s) - np.float64(lo))                  # a difference of float32 values, rounded once
        scaled = F32(np.float64(offset) * np.float64(scale))
        out.append(min(int(scaled), bins - 1))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def golden_histogram(name, key, bins):
    frame = np.load(os.path.join(GOLD, name + ".npz"))[key].astype(F32)
    lo, hi, _ = ref.value_range(frame)
    counts, info = ref.histogram(frame, lo, hi, bins)
    assert info["used"] == frame.size
    counts.setflags(write=False)
    return counts


GOLDEN = [("inputs_128", "frame_0"), ("inputs_128", "frame_1"), ("inputs_rub", "slice_0"), ("inputs_rub", "slice_1")]
NAMED = {"two-valued": [0, 4, 0, 0, 9, 0], "three-valued": [3, 0, 5, 0, 0, 7], "single-bin": [0, 0, 11, 0], "empty": [0, 0, 0, 0],
         "one-bin-wide": [5], "symmetric": [5, 1, 0, 0, 1, 5], "flat": [2] * 9, "ties": [1, 0, 0, 0, 1, 0, 0, 0, 1]}


# ---- the restatement against independent forms ------------------------------------------------------------------------------------------

def test_the_bin_rule_is_monotone_and_counts_are_its_bincount():
    rng = np.random.default_rng(1)
    for lo, hi, bins in ((0.0, 1.0, 256), (-3.5, 7.25, 1000), (0.0, 255.0, 256), (7.0, 243.0, 64), (-1e-3, 1e-3, 4096), (0.1, 0.7, 1)):
        v = np.sort(rng.uniform(lo, hi, 20000).astype(F32))
        v = v[(v >= F32(lo)) & (v <= F32(hi))]
        b = ref.bin_of(v, lo, hi, bins)
        assert (np.diff(b) >= 0).all() and b.min() >= 0 and b.max() <= bins - 1
        assert ref.bin_of(F32(hi), lo, hi, bins) == bins - 1 and ref.bin_of(F32(lo), lo, hi, bins) == 0
        shuffled = rng.permutation(v).reshape(1, 1, -1)
        counts, info = ref.histogram(shuffled, lo, hi, bins)
        assert np.array_equal(counts, np.bincount(b, minlength=bins)) and info["used"] == len(v)
        # counts through the edges: bin k holds the values in [edge(k), edge(k + 1))
        for k in sorted({0, 1, bins // 3, bins - 1}):
            if k < bins:
                above = (v >= ref.edge(lo, hi, bins, k)).sum()
                assert above == counts[k:].sum(), (lo, hi, bins, k)


@pytest.mark.parametrize("bins", [1, 2, 7, 4096])
def test_the_bin_rule_against_every_float_of_a_narrow_range(bins):
    values = narrow_floats()
    got = ref.bin_of(values, *NARROW, bins)
    assert np.array_equal(got, exact_bins(values, *NARROW, bins))
    assert got[0] == 0 and got[-1] == bins - 1 and (np.diff(got) >= 0).all()
    assert len(np.unique(got)) == min(bins, 4096)                      # 8192 steps: every one of up to 4096 bins occurs


def test_the_counters_and_the_range_of_the_special_values():
    v = np.array([[[np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 0.25, 0.75, np.nextafter(F32(0.75), F32(1)),
                    np.nextafter(F32(0.25), F32(0)), 0.5]]], F32)
    counts, info = ref.histogram(v, 0.25, 0.75, 2)
    assert info == dict(masked=0, nan=1, below=6, above=2, used=3) and counts.tolist() == [1, 2]       # 0.5 and hi in the last bin
    mask = np.ones(v.shape, np.int32)
    mask[0, 0, [0, 1, 7]] = 0
    mask[0, 0, 8] = -5                                                  # a negative value lets the voxel through
    counts, info = ref.histogram(v, 0.25, 0.75, 2, mask)
    assert info == dict(masked=3, nan=0, below=6, above=1, used=2) and counts.tolist() == [0, 2]
    lo, hi, rinfo = ref.value_range(v)
    assert rinfo == dict(masked=0, nan=1, infinite=2, finite=9) and lo == F32(-1e-45) and hi == np.nextafter(F32(0.75), F32(1))
    zeros = np.array([[[0.0, -0.0, np.nan]]], F32)
    lo, hi, _ = ref.value_range(zeros)
    assert np.signbit(lo) and not np.signbit(hi) and lo == 0 and hi == 0                                # -0.0 is below +0.0
    lo, hi, rinfo = ref.value_range(np.array([[[np.nan, np.inf]]], F32))
    assert lo == np.inf and hi == -np.inf and rinfo["finite"] == 0
    denormal = np.array([[[1e-45, 3e-45, 1e-40]]], F32)
    assert ref.value_range(denormal)[:2] == (F32(1e-45), F32(1e-40))                                   # a denormal keeps its value


# ---- f3d_histogram_edge -------------------------------------------------------------------------------------------------------------------

def host_edge(f3d, lo, hi, bins, k):
    edge = C.c_float(-7.0)
    status = f3d.host().f3d_histogram_edge(float(lo), float(hi), bins, k, C.byref(edge))
    return status, F32(edge.value)


@pytest.mark.parametrize("bins", [1, 2, 7, 4096])
def test_the_edge_against_a_brute_force_over_every_float(f3d, bins):
    values = narrow_floats()
    b = exact_bins(values, *NARROW, bins)
    for k in range(bins):
        want = values[np.argmax(b >= k)]                               # the first float whose bin is at least k
        status, got = host_edge(f3d, *NARROW, bins, k)
        assert status == 0 and got.tobytes() == want.tobytes(), k
        if bins <= 7 or k % 97 == 0:                                   # the restatement's bisection, too (slower)
            assert ref.edge(*NARROW, bins, k).tobytes() == want.tobytes()
        if k:
            assert ref.bin_of(np.nextafter(got, F32(-np.inf)), *NARROW, bins) < k
    assert host_edge(f3d, *NARROW, bins, 0)[1] == NARROW[0]


def test_the_edge_on_the_ranges_of_the_frames(f3d):
    for lo, hi, bins in ((0.0, 255.0, 256), (7.0, 243.0, 64), (0.0, 255.0, 64), (-1.0, 1.0, 1000)):
        for k in range(bins):
            status, got = host_edge(f3d, lo, hi, bins, k)
            assert status == 0 and got.tobytes() == ref.edge(lo, hi, bins, k).tobytes()
            assert ref.bin_of(got, lo, hi, bins) >= k
            if k:
                assert ref.bin_of(np.nextafter(got, F32(-np.inf)), lo, hi, bins) < k


def test_the_edge_refuses(f3d):
    for lo, hi, bins, k in ((1, 1, 4, 0), (2, 1, 4, 0), (np.nan, 1, 4, 0), (0, np.inf, 4, 0), (-np.inf, 0, 4, 0), (0, 1, 0, 0), (0, 1, 4097, 0),
                            (0, 1, 4, 4), (-3e38, 3e38, 4, 0), (0, 1e-45, 4096, 0)):
        status, got = host_edge(f3d, lo, hi, bins, k)
        assert status != 0 and got == F32(-7.0) and b"f3d_histogram_edge" in f3d.host().f3d_host_last_error()


# ---- f3d_otsu -----------------------------------------------------------------------------------------------------------------------------

def host_otsu(f3d, counts, classes):
    counts = np.ascontiguousarray(counts, np.uint64)
    cuts = (C.c_uint * 2)(77, 77)
    info = f3d.OtsuInfo()
    status = f3d.host().f3d_otsu(counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), len(counts), classes, cuts, C.byref(info))
    assert status == 0, f3d.host().f3d_host_last_error()
    return info.status, list(cuts), list(info.populations), info.objective


def check_otsu(f3d, counts, classes):
    status, cuts, populations, objective = host_otsu(f3d, counts, classes)
    want = ref.otsu(counts, classes)
    assert status == want[0]
    if status == ref.OTSU_DEGENERATE:
        assert cuts == [77, 77] and populations == [0, 0, 0] and objective == 0.0
        return None
    assert cuts[:classes - 1] == want[1] and cuts[classes - 1:] == [77] * (3 - classes)
    assert populations[:classes] == want[2] and sum(populations[:classes]) == int(np.sum(counts, dtype=np.uint64))
    assert np.float64(objective).tobytes() == np.float64(want[3]).tobytes()
    assert ref.otsu_objective(counts, want[1]) == want[3]
    return want[1]


@pytest.mark.parametrize("bins,classes", [(256, 2), (64, 2), (64, 3)])
@pytest.mark.parametrize("name,key", GOLDEN)
def test_otsu_of_the_golden_frames_equals_the_restatement(f3d, name, key, bins, classes):
    cuts = check_otsu(f3d, golden_histogram(name, key, bins), classes)
    if (name, key, bins, classes) == ("inputs_128", "frame_0", 256, 2):
        assert cuts == [85]


@pytest.mark.parametrize("case", sorted(NAMED))
@pytest.mark.parametrize("classes", [2, 3])
def test_otsu_of_the_named_histograms(f3d, case, classes):
    counts = NAMED[case]
    cuts = check_otsu(f3d, counts, classes)
    occupied = sum(c != 0 for c in counts)
    assert (cuts is None) == (occupied < classes)
    if case == "two-valued" and classes == 2:
        assert cuts == [2]                                              # every cut between the two values ties: the smallest wins
    if case == "symmetric" and classes == 2:
        assert cuts == [2]                                              # cuts 2, 3 and 4 give the same classes
    if case == "three-valued" and classes == 3:
        assert cuts == [1, 3]
    if case == "ties" and classes == 3:
        assert cuts == [1, 5]


def test_otsu_of_random_histograms_with_ties(f3d):
    rng = np.random.default_rng(3)
    for trial in range(60):
        bins = int(rng.integers(1, 40))
        counts = rng.integers(0, 4 if trial % 2 else 10 ** 6, bins) * (rng.random(bins) < 0.6)
        for classes in (2, 3):
            check_otsu(f3d, counts.astype(np.uint64), classes)


def exact_objective(counts, cuts):
    bounds = [0] + list(cuts) + [len(counts)]
    total = Fraction(0)
    for a, b in zip(bounds[:-1], bounds[1:]):
        n = sum(int(c) for c in counts[a:b])
        if n == 0:
            return None
        m = sum(i * int(counts[i]) for i in range(a, b))
        total += Fraction(m * m, n)
    return total


def exact_argmax(counts, classes):
    bins = len(counts)
    candidates = [(c,) for c in range(1, bins)] if classes == 2 else [(a, b) for a in range(1, bins - 1) for b in range(a + 1, bins)]
    scored = [(exact_objective(counts, c), c) for c in candidates]
    scored = [(v, c) for v, c in scored if v is not None]
    best = max(v for v, _ in scored)
    return best, [c for v, c in scored if v == best], sorted((v for v, _ in scored), reverse=True)


@pytest.mark.parametrize("bins,classes", [(256, 2), (64, 2), (64, 3)])
@pytest.mark.parametrize("name,key", GOLDEN[::2])
def test_otsu_against_exact_arithmetic_on_the_golden_frames(f3d, name, key, bins, classes):
    counts = golden_histogram(name, key, bins)
    status, cuts, _, objective = host_otsu(f3d, counts, classes)
    best, at, ranked = exact_argmax(counts, classes)
    chosen = exact_objective(counts, cuts[:classes - 1])
    assert status == ref.OTSU_OK and chosen >= (1 - Fraction(1, 2 ** 49)) * best
    assert at == [tuple(cuts[:classes - 1])]                            # on these frames the chosen cut IS the exact argmax
    assert abs(Fraction(objective) - chosen) <= 5 * Fraction(1, 2 ** 53) * chosen
    print(name, key, bins, classes, "runner-up lower by", float((ranked[0] - ranked[1]) / ranked[0]))


def test_otsu_against_exact_arithmetic_on_random_histograms(f3d):
    rng = np.random.default_rng(9)
    for trial in range(40):
        bins = int(rng.integers(3, 24))
        counts = (rng.integers(1, 2 ** 28, bins) * (rng.random(bins) < 0.8)).astype(np.uint64)      # at most 23 * 2^28 < 2^33 voxels
        for classes in (2, 3):
            status, cuts, _, _ = host_otsu(f3d, counts, classes)
            if status == ref.OTSU_OK:
                best, _, _ = exact_argmax(counts, classes)
                assert exact_objective(counts, cuts[:classes - 1]) >= (1 - Fraction(1, 2 ** 49)) * best


def test_otsu_refuses(f3d):
    host = f3d.host()
    counts = np.array([1, 2, 3], np.uint64)
    ptr = counts.ctypes.data_as(C.POINTER(C.c_ulonglong))
    cuts, info = (C.c_uint * 2)(77, 77), f3d.OtsuInfo()
    info.status = 55
    for bins, classes, c, i in ((3, 4, cuts, info), (3, 1, cuts, info), (0, 2, cuts, info), (4097, 2, cuts, info), (3, 2, None, info),
                                (3, 2, cuts, None)):
        assert host.f3d_otsu(ptr, bins, classes, c, C.byref(i) if i is not None else None) != 0
        assert b"f3d_otsu" in host.f3d_host_last_error()
    huge = np.array([2 ** 33, 1], np.uint64)
    assert host.f3d_otsu(huge.ctypes.data_as(C.POINTER(C.c_ulonglong)), 2, 2, cuts, C.byref(info)) != 0
    assert b"2^33" in host.f3d_host_last_error()
    assert list(cuts) == [77, 77] and info.status == 55


# ---- f3d_histogram_rank -------------------------------------------------------------------------------------------------------------------

def test_the_rank_against_searchsorted(f3d):
    host = f3d.host()
    rng = np.random.default_rng(5)
    for trial in range(30):
        bins = int(rng.integers(1, 300))
        counts = (rng.integers(0, 50, bins) * (rng.random(bins) < 0.5)).astype(np.uint64)
        ptr = counts.ctypes.data_as(C.POINTER(C.c_ulonglong))
        used = int(counts.sum())
        cumulative = np.cumsum(counts)
        found = C.c_uint(9999)
        for r in sorted({0, used // 3, used // 2, used - 1} | set(rng.integers(0, max(used, 1), 20).tolist())):
            if 0 <= r < used:
                assert host.f3d_histogram_rank(ptr, bins, r, C.byref(found)) == 0
                assert found.value == np.searchsorted(cumulative, r, side="right") == ref.rank(counts, r)
        found = C.c_uint(9999)
        assert host.f3d_histogram_rank(ptr, bins, used, C.byref(found)) != 0 and found.value == 9999
        assert b"f3d_histogram_rank" in host.f3d_host_last_error()
    h = f3d.Histogram(np.array([0, 3, 0, 1], np.uint64), 0.0, 1.0, {})
    assert [h.rank(r) for r in range(4)] == [1, 1, 1, 3] and h.quantile(0) == 1 and h.quantile(1) == 3 and h.quantile(0.5) == 1


# ---- the host functions under sanitizers ----------------------------------------------------------------------------------------------------

def test_the_host_functions_in_a_program_under_sanitizers(tmp_path):
    """host/threshold_select.cpp with tests/histogram_host_main.cpp, a program of its own, built with -fsanitize=address,undefined and
    run here on the CPU; nothing loaded into python runs under a sanitizer"""
    exe = tmp_path / "histogram_host"
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cuda-flow3d_amd", "host"),
                    os.path.join(ROOT, "tests", "histogram_host_main.cpp"),
                    os.path.join(ROOT, "cuda-flow3d_amd", "host", "threshold_select.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok histogram host"), (run.stdout[-2000:], run.stderr[-3000:])
    assert run.stdout.count(" 0 wrong") == 8 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_the_header(f3d, tmp_path):
    structs = {"f3d_histogram_info": (f3d.HistogramInfo, ref.HISTOGRAM_INFO), "f3d_range_info": (f3d.RangeInfo, ref.RANGE_INFO),
               "f3d_otsu_info": (f3d.OtsuInfo, ("status", "populations", "objective"))}
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("%zu\\n", sizeof({s}));\n' + "".join(f'  printf("%zu\\n", offsetof({s}, {n}));\n' for n in names)
                   for s, (_, names) in structs.items())
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "f3d_host.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for T, names in structs.values():
        assert [n for n, _ in T._fields_] == list(names)
        want += [C.sizeof(T)] + [getattr(T, n).offset for n in names]
    assert got == want == [40, 0, 8, 16, 24, 32, 32, 0, 8, 16, 24, 40, 0, 8, 32]


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_histogram", "f3d_value_range"]),
                                              ("f3d_host.h", "host", ["f3d_histogram_edge", "f3d_otsu", "f3d_histogram_rank",
                                                                      "f3d_flow_histogram"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    needles = {"f3d.h": ("lo <= s && s <= hi", "min((int)((s - lo) * scale), bins - 1)", "sum(counts) == used", "-0.0f is below +0.0f",
                         "min is +inf and max is -inf", "bins outside 1 .. 4096"),
               "f3d_host.h": ("smallest float32 s in [lo, hi] whose bin is at least k", "(double)M * (double)M / (double)N",
                              "ties go to the smallest cut", "F3D_OTSU_DEGENERATE", "refused\n * at r >= used")}[header]
    for needle in needles:
        assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    assert len(f3d._histogram_entry().argtypes) == 10 and len(f3d._value_range_entry().argtypes) == 8
    good = np.zeros((3, 4, 5), F32)
    for bins in (0, 4097, -1, 2.5):
        with pytest.raises(ValueError, match="bins"):
            f3d.histogram(good, bins=bins)
    for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (1.0,), "ab", 3):
        with pytest.raises(ValueError, match="range"):
            f3d.histogram(good, range=bad)
    for bad in (np.zeros((4, 5), F32), np.zeros((0, 4, 5), F32)):
        with pytest.raises(ValueError, match="volume"):
            f3d.histogram(bad, range=(0, 1))
        with pytest.raises(ValueError, match="volume"):
            f3d.value_range(bad)
    with pytest.raises(ValueError, match="mask"):
        f3d.histogram(good, range=(0, 1), mask=np.ones((3, 4, 6), np.int32))
    with pytest.raises(ValueError, match="mask"):
        f3d.value_range(good, mask=np.ones((3, 4, 5), F32))
    host = f3d.host()
    counts, info, lo, hi = np.zeros(4, np.uint64), f3d.HistogramInfo(), C.c_float(), C.c_float()
    assert host.f3d_flow_histogram(None, 0, None, 4, counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info), C.byref(lo), C.byref(hi)) != 0
    assert b"f3d_flow_histogram" in host.f3d_host_last_error()
    assert hasattr(f3d.OpticalFlow, "histogram")
    h = f3d.Histogram(np.array([1, 0, 2], np.uint64), 0.0, 3.0, dict.fromkeys(ref.HISTOGRAM_INFO, 0))
    assert h.bins == 3 and h.edge(0) == 0 and h.edge(2) == 2 and h.otsu().cuts.tolist() == [1] and h.otsu().values.tolist() == [1.0]
    assert h.otsu(3).status == f3d.OTSU_DEGENERATE and len(h.otsu(3).cuts) == 0
    for classes in (1, 4):
        with pytest.raises(ValueError, match="classes"):
            h.otsu(classes)
    with pytest.raises(f3d.F3dError, match="f3d_histogram_edge"):
        h.edge(3)
    with pytest.raises(ValueError, match="q must"):
        h.quantile(1.5)
    flow = f3d.OpticalFlow.__new__(f3d.OpticalFlow)                  # no device: the checks come before any call
    for lo, hi, needle in (("otsu", "otsu2", "mixed"), ("otsu2", "otsu1", "above"), ("otsu", "otsu", "above"), ("median", 1.0, "numbers or one of")):
        with pytest.raises(ValueError, match=needle):
            flow._otsu_bounds(lo, hi, 256, None)
    assert flow._otsu_bounds(0.25, 0.5, 256, None) == (0.25, 0.5)


CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    u, v, w = flow.download()
    for call in (lambda: flow.histogram(), lambda: flow.histogram(16, (0.0, 1.0)), lambda: flow.segment("otsu"),
                 lambda: pkg.histogram(f0, range=(0.0, 1.0))):
        try:
            call(); raise SystemExit("a call succeeded without f3d_histogram")
        except pkg.F3dError as e:
            assert "f3d_histogram" in str(e), str(e)
    try:
        pkg.value_range(f0); raise SystemExit("a call succeeded without f3d_value_range")
    except pkg.F3dError as e:
        assert "f3d_value_range" in str(e), str(e)
    h = pkg.Histogram(np.array([4, 0, 0, 9], np.uint64), 0.0, 1.0, {})          # the host functions need no device entry
    assert h.otsu().cuts.tolist() == [1] and h.edge(1) == 0.25 and h.rank(4) == 3
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_histogram nor f3d_value_range: libf3d_host.so built against it must still load (RTLD_NOW)
    and solve flows, and ComputeHistogram must fail with a message naming f3d_histogram"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_histogram" not in names and "f3d_value_range" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


REFUSALS = {
    "mixed": (["--segment", "otsu:otsu2"], "cannot be mixed"), "mixed-reversed": (["--segment", "otsu1:otsu"], "cannot be mixed"),
    "upper-below-lower": (["--segment", "otsu2:otsu1"], "LO is above HI"), "same-cut": (["--segment", "otsu:otsu"], "LO is above HI"),
    "unknown-token": (["--segment", "median:"], "usage"), "unknown-token-hi": (["--segment", ":otsu3"], "usage"),
    "capital": (["--segment", "Otsu:"], "usage"),
    "bins-zero": (["--segment", "otsu:", "--segment-bins", "0"], "usage"), "bins-above": (["--segment", "otsu:", "--segment-bins", "4097"], "usage"),
    "bins-word": (["--segment", "otsu:", "--segment-bins", "many"], "usage"), "bins-negative": (["--segment", "otsu:", "--segment-bins", "-4"], "usage"),
    "bins-missing": (["--segment", "otsu:", "--segment-bins"], "usage"),
    "bins-without-token": (["--segment", "0.4:", "--segment-bins", "64"], "they need otsu"),
    "bins-alone": (["--segment-bins", "64"], "they need otsu"), "range-without-token": (["--segment", "0.4:", "--segment-range", "0:1"], "they need otsu"),
    "range-empty": (["--histogram", "--segment-range", ""], "usage"), "range-half": (["--histogram", "--segment-range", "0.5:"], "usage"),
    "range-other-half": (["--histogram", "--segment-range", ":0.5"], "usage"), "range-no-colon": (["--histogram", "--segment-range", "0.5"], "usage"),
    "range-two-colons": (["--histogram", "--segment-range", "0:1:2"], "usage"), "range-word": (["--histogram", "--segment-range", "a:b"], "usage"),
    "range-nan": (["--histogram", "--segment-range", "nan:1"], "usage"), "range-inf": (["--histogram", "--segment-range", "0:inf"], "usage"),
    "range-reversed": (["--histogram", "--segment-range", "1:0"], "A must be below B"),
    "range-equal": (["--histogram", "--segment-range", "1:1"], "A must be below B"),
    "range-missing": (["--histogram", "--segment-range"], "usage"),
    "histogram-partial": (["--histogram", "--partial"], "--histogram needs the resident"),
    "histogram-concurrent": (["--histogram", "--concurrent", "2"], "--histogram needs the resident"),
    "token-with-labels": (["--segment", "otsu:", "--labels", "LABELS", "--contacts"], "--segment takes the place of --labels"),
    "token-partial": (["--segment", ":otsu", "--partial"], "--segment needs the resident"),
    "token-lo-above-number": (["--segment", "0.5:0.25"], "LO is above HI"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_flow3d_refuses_before_any_device_is_touched(tmp_path, case):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(2):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    good = tmp_path / "labels.raw"
    np.ones(64, np.int32).tofile(good)
    extra, needle = REFUSALS[case]
    extra = [str(good) if a == "LABELS" else a for a in extra]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--segment-bins B] [--segment-range A:B]" in run.stdout and "[--histogram]" in run.stdout
    assert "[--segment LO:HI [--segment-min-voxels K]]" in run.stdout                            # the earlier usage text is all there
    assert "3D optical flow" not in run.stdout                                                   # before any device is touched
    assert not any("histogram" in n or "bodies" in n or "flow-" in n or (n.endswith("labels.raw") and n != "labels.raw")
                   for n in os.listdir(tmp_path))
