"""Statistics of a field per labelled body without a GPU: the numpy restatement (tests/label_field_ref.py) against a loop over the voxels,
label by label; the quantisation at its edges; the bins; the host solve (f3d_label_field_solve) bit for bit against the restatement's
evaluation from Python integers; the solve under AddressSanitizer and UBSan in a stand-alone program; the struct layouts; the binding's
argument checks; the automatic shift; the message of a device library without the new entries; and the refusals of bin/flow3d
--label-stats.

Bounds.  The sums are exact integers and the solve is a fixed sequence of binary64 operations on exact integers, each rounded once:
equality of the bytes throughout."""
import ctypes as C
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import label_field_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
HOST = os.path.join(ROOT, "cuda-flow3d_amd", "host")
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [0, 1, 7, 256])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (3, 4, 5), (6, 5, 7)], ids=str)
def test_the_restatement_against_a_loop_over_the_voxels(shape, bins):
    rng = np.random.default_rng(sum(shape) + bins)
    labels = rng.integers(-1, 5, shape).astype(np.int32)              # background, foreign on both sides (-1 and 4), three bodies
    field = ref.case_field(shape[::-1], "noise")
    fast, counts, info = ref.label_field_sums(field, labels, 3, 14, -500.0, 750.5, bins)
    slow, slow_counts = ref.loops(field, labels, 3, 14, -500.0, 750.5, bins)
    assert fast.tobytes() == slow.tobytes()
    assert (counts is None and slow_counts is None) if bins == 0 else np.array_equal(counts, slow_counts)
    assert sum(info.values()) == np.prod(shape) and int(fast["n"].sum()) == info["used"]
    spare, _, _ = ref.label_field_sums(field, labels, 6, 14, -500.0, 750.5, bins)
    assert spare[:3].tobytes() == fast.tobytes() and (spare["n"][4:] == 0).all()
    assert (spare["min_key"][4:] == 0xFFFFFFFF).all() and (spare["max_key"][4:] == 0).all()


def one(values, shift, lo=0.0, hi=0.0, bins=0):
    """(the row of label 1, its counts, info) of a row of values"""
    v = np.asarray(values, F32).reshape(1, 1, -1)
    rows, counts, info = ref.label_field_sums(v, np.ones(v.shape, np.int32), 1, shift, lo, hi, bins)
    return rows[0], None if counts is None else counts[0], info


def test_quantisation_ties_go_to_even_for_both_signs():
    row, _, info = one([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5], 0)
    assert info["used"] == 7 and int(row["iq"]) == 0 + 2 + 2 - 0 - 2 - 2 + 4
    assert int(row["iqq_lo"]) == 4 + 4 + 4 + 4 + 16 and int(row["iqq_hi"]) == 0
    row, _, _ = one([0.5 / 16, 1.5 / 16, -2.5 / 16], 4)                   # a positive shift
    assert int(row["iq"]) == 0 + 2 - 2
    row, _, _ = one([20.0, 28.0, -12.0], -3)                              # a negative one: 2.5, 3.5, -1.5
    assert int(row["iq"]) == 2 + 4 - 2


def test_the_edge_of_the_range_infinities_nan_and_denormals():
    edge = F32(2.0 ** 24)
    beyond = np.nextafter(edge, F32(np.inf))
    row, _, info = one([edge, -edge, beyond, -beyond, np.inf, -np.inf, np.nan, 1e-40, -1e-40], 0)
    assert info == dict(background=0, foreign=0, nan=1, out_of_range=4, used=4)
    assert int(row["n"]) == 4 and int(row["iq"]) == 0 and (int(row["iqq_hi"]) << 32) + int(row["iqq_lo"]) == 2 * 2 ** 48
    assert int(row["iqq_hi"]) == 2 ** 17 and int(row["iqq_lo"]) == 0     # the high limb
    assert ref.href.float_of_key(np.uint32(int(row["min_key"])))[()] == -edge and ref.href.float_of_key(np.uint32(int(row["max_key"])))[()] == edge
    row, _, info = one([1e-40, 3e-45, 0.0], 100)                          # denormals keep their value: 1e-40 * 2^100 is about 1.27e-10
    assert info["used"] == 3 and int(row["iq"]) == 0
    assert ref.href.float_of_key(np.uint32(int(row["max_key"])))[()] == F32(1e-40) and int(row["min_key"]) == 0x80000000
    row, _, info = one([F32(1e-40)], -100)                                # the product underflows to zero: still one float32 product
    assert info["used"] == 1 and int(row["iq"]) == 0


def test_minus_zero_is_below_plus_zero():
    row, _, _ = one([0.0, -0.0], 0)
    assert int(row["min_key"]) == 0x7FFFFFFF and int(row["max_key"]) == 0x80000000
    stats, _ = ref.solve(np.array([row]), None, 0)
    assert math.copysign(1.0, stats["min"][0]) == -1.0 and math.copysign(1.0, stats["max"][0]) == 1.0


def test_the_bins_add_up_and_hi_lands_in_the_last_bin():
    values = [1.0, 1.25, 2.0, 3.0, 0.5, 3.5, 3.0, np.nextafter(F32(3.0), F32(4)), np.nextafter(F32(1.0), F32(0))]
    row, counts, info = one(values, 4, 1.0, 3.0, 4)
    assert int(row["below"]) == 2 and int(row["above"]) == 2 and counts.tolist() == [2, 0, 1, 2]
    assert int(row["below"]) + int(row["above"]) + int(counts.sum()) == int(row["n"]) == info["used"] == 9
    full = ref.case_field((9, 8, 7), "noise")
    labels = np.random.default_rng(3).integers(0, 4, full.shape).astype(np.int32)
    for bins in (1, 64, 256):
        rows, counts, _ = ref.label_field_sums(full, labels, 3, 14, -500.0, 750.5, bins)
        assert np.array_equal(rows["below"] + rows["above"] + counts.sum(axis=1).astype(np.uint64), rows["n"])
        hist, _ = ref.href.histogram(full, -500.0, 750.5, bins, mask=(labels == 2))
        assert counts[1].astype(np.uint64).tolist() == hist.tolist()       # the bin function is the histogram's


# ---- the host solve ----------------------------------------------------------------------------------------------------------------------

def as_sums(f3d, rows, counts, shift, lo, hi):
    bins = 0 if counts is None else counts.shape[1]
    return f3d.LabelFieldSums(rows, counts, shift, float(F32(lo)) if bins else None, float(F32(hi)) if bins else None, {})


def row_of(n, iq, iqq, low=1.0, high=1.0):
    r = np.zeros(1, ref.SUMS_DTYPE)
    r["n"], r["iq"], r["iqq_lo"], r["iqq_hi"] = n, iq, iqq & 0xFFFFFFFF, iqq >> 32
    r["min_key"] = int(ref.href.key_of(F32(low)).ravel()[0]) if n else 0xFFFFFFFF
    r["max_key"] = int(ref.href.key_of(F32(high)).ravel()[0]) if n else 0
    return r


def test_the_solve_bit_for_bit_against_python_integers(f3d):
    rng = np.random.default_rng(11)
    for shift, lo, hi, bins, min_voxels in ((14, -500.0, 750.5, 64, 20), (-3, -1.0e6, 2.0e6, 256, 1), (8, 0.0, 65535.0, 1, 1), (10, 0.0, 0.0, 0, 30)):
        kind = {14: "noise", -3: "ties", 8: "integers", 10: "ramp"}[shift]
        field = ref.case_field((21, 13, 9), kind)
        labels = rng.integers(0, 9, field.shape).astype(np.int32)
        labels[labels == 7] = 0                                           # an empty label
        labels[(labels == 5) & (rng.random(field.shape) < 0.97)] = 0       # a small one
        rows, counts, _ = ref.label_field_sums(field, labels, 8, shift, lo, hi, bins)
        want, summary = ref.solve(rows, counts, shift, lo, hi, bins, min_voxels)
        got = f3d.solve_label_field(as_sums(f3d, rows, counts, shift, lo, hi), min_voxels)
        assert got.rows.tobytes() == want.tobytes(), [n for n in ref.STAT_DTYPE.names if got.rows[n].tobytes() != want[n].tobytes()]
        assert got.summary["mean"] == summary["mean"] and [got.summary[k] for k in ("ok", "empty", "small")] == [summary[k] for k in ("ok", "empty", "small")]
        assert want["status"][6] == ref.EMPTY and (min_voxels == 1 or ref.SMALL in want["status"]) and (want["status"] == ref.OK).any()
        assert math.isnan(got.mean[6]) and math.isnan(got.min[6]) and got.q05_bin[6] == -1
        if bins == 0:
            assert np.isnan(got.median).all() and (got.median_bin == -1).all() and got.counts is None
    # against numpy's float64 statistics of the quantised values: the mean to a rounding, the deviation to a few
    field = ref.case_field((21, 13, 9), "ramp")
    rows, _, _ = ref.label_field_sums(field, np.ones(field.shape, np.int32), 1, 10)
    got = f3d.solve_label_field(as_sums(f3d, rows, None, 10, 0, 0))
    assert got.mean[0] == pytest.approx(field.astype(np.float64).mean(), rel=1e-13)
    assert got.std[0] == pytest.approx(field.astype(np.float64).std(), rel=1e-12) and got.variance[0] == pytest.approx(got.std[0] ** 2, rel=1e-15)
    assert (got.min[0], got.max[0]) == (float(field.min()), float(field.max()))


def test_the_high_limb_and_a_variance_of_exactly_zero(f3d):
    q, n = 2 ** 24, 2 ** 31 - 1
    big = row_of(n, 0, n * q * q, -1.0, 1.0)                               # n voxels at +-2^24 quanta: iqq = (2^31 - 1) 2^48 needs the high limb
    assert int(big["iqq_hi"][0]) >= 2 ** 32
    constant = row_of(12345, 12345 * 52, 12345 * 52 * 52, 3.25, 3.25)      # 3.25 at shift 4
    n1, n2, q1, q2 = 2 ** 30, 2 ** 30 - 1, 2 ** 24 - 1, 2 ** 24 - 3           # iq above 2^53 and odd: its conversion rounds before the division
    odd = row_of(n1 + n2, n1 * q1 + n2 * q2, n1 * q1 * q1 + n2 * q2 * q2)
    assert int(odd["iq"][0]) > 2 ** 54 and int(odd["iq"][0]) % 2 == 1
    rows = np.concatenate([big, constant, odd])
    want, _ = ref.solve(rows, None, 4)
    got = f3d.solve_label_field(as_sums(f3d, rows, None, 4, 0, 0))
    assert got.rows.tobytes() == want.tobytes()
    assert got.variance[1] == 0.0 and got.std[1] == 0.0 and got.mean[1] == 3.25
    assert got.std[0] == 2.0 ** 20 and got.mean[0] == 0.0


@pytest.mark.parametrize("m,ranks", [(1, (0, 0, 0)), (2, (0, 0, 1)), (19, (0, 9, 18)), (20, (0, 9, 19)), (21, (1, 10, 19))])
def test_the_three_ranks(f3d, m, ranks):
    counts = np.zeros((1, 32), np.uint32)
    counts[0, :m] = 1                                                     # the voxel of rank r lies in bin r
    rows = row_of(m, m, m)
    got = f3d.solve_label_field(as_sums(f3d, rows, counts, 0, 0.0, 32.0))
    want, _ = ref.solve(rows, counts, 0, 0.0, 32.0, 32)
    assert got.rows.tobytes() == want.tobytes()
    assert (int(got.q05_bin[0]), int(got.median_bin[0]), int(got.q95_bin[0])) == ranks
    assert (got.q05[0], got.median[0], got.q95[0]) == tuple(r + 0.5 for r in ranks)


def test_a_quantile_is_the_midpoint_of_float32_edges(f3d):
    lo, hi, bins = 0.1, 0.7, 7                                            # edges that are not representable: bisection decides them
    counts = np.zeros((1, bins), np.uint32)
    counts[0, 3], counts[0, 6] = 5, 1
    got = f3d.solve_label_field(as_sums(f3d, row_of(6, 6, 6), counts, 0, lo, hi))
    e3, e4, e6 = (float(ref.href.edge(F32(lo), F32(hi), bins, k)) for k in (3, 4, 6))
    assert got.median[0] == (e3 + e4) / 2.0 and got.q95[0] == (e6 + float(F32(hi))) / 2.0 and got.q05_bin[0] == 3


def test_the_solve_under_the_sanitizers(tmp_path):
    """host/label_field.cpp, host/threshold_select.cpp and tests/label_field_solve_main.cpp built into a program of their own with
    AddressSanitizer and UBSan"""
    exe = tmp_path / "label_field_solve"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(HOST, "label_field.cpp"), os.path.join(HOST, "threshold_select.cpp"),
                    os.path.join(ROOT, "tests", "label_field_solve_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-2000:], run.stderr[-3000:])


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_the_header(f3d, tmp_path):
    src = tmp_path / "sizes.c"
    sums = ("min_key", "max_key", "iq", "iqq_lo", "iqq_hi", "below", "above")
    stat = ("q05_bin", "median_bin", "q95_bin", "n", "below", "above", "min", "max", "mean", "variance", "std", "q05", "median", "q95")
    lines = ['printf("%zu' + ' %zu' * len(sums) + '\\n", sizeof(struct f3d_label_field_sums), ' +
             ", ".join(f"offsetof(struct f3d_label_field_sums, {n})" for n in sums) + ");",
             'printf("%zu %zu %zu\\n", sizeof(f3d_label_field_info), offsetof(f3d_label_field_info, out_of_range), offsetof(f3d_label_field_info, used));',
             'printf("%zu' + ' %zu' * len(stat) + '\\n", sizeof(f3d_label_field_stat), ' +
             ", ".join(f"offsetof(f3d_label_field_stat, {n})" for n in stat) + ");",
             'printf("%zu %zu %zu\\n", sizeof(f3d_label_field_summary), offsetof(f3d_label_field_summary, small), offsetof(f3d_label_field_summary, mean));',
             'printf("%d %d %d\\n", F3D_LABEL_OK, F3D_LABEL_EMPTY, F3D_LABEL_SMALL);']
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"f3d_host.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    S, I, T, U = f3d.LabelFieldSumsRow, f3d.LabelFieldInfo, f3d.LabelFieldStat, f3d.LabelFieldSummary
    assert out[0] == [C.sizeof(S)] + [getattr(S, n).offset for n in sums] == [64, 8, 16, 24, 32, 40, 48, 56]
    assert out[1] == [C.sizeof(I), I.out_of_range.offset, I.used.offset] == [40, 24, 32]
    assert out[2] == [C.sizeof(T)] + [getattr(T, n).offset for n in stat] == [104, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert out[3] == [C.sizeof(U), U.small.offset, U.mean.offset] == [32, 16, 24]
    assert out[4] == [ref.OK, ref.EMPTY, ref.SMALL] == [f3d.LABEL_STATUS.index(k) for k in ("ok", "empty", "small")]
    assert f3d._FIELD_SUMS_DTYPE == ref.SUMS_DTYPE and f3d._FIELD_STAT_DTYPE == ref.STAT_DTYPE
    for name in ref.SUMS_DTYPE.names:
        assert ref.SUMS_DTYPE.fields[name][1] == getattr(S, name).offset, name
    for name in ref.STAT_DTYPE.names:
        assert ref.STAT_DTYPE.fields[name][1] == getattr(T, name).offset, name


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_label_field_sums", "f3d_paint_labels"]),
                                              ("f3d_host.h", "host", ["f3d_label_field_solve", "f3d_label_field_shift", "f3d_flow_label_field_compute",
                                                                      "f3d_flow_label_field_range", "f3d_flow_field_container", "f3d_flow_labels_paint"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    needles = (("ONE float32 product with scale = ldexpf(1.0f, shift)", "fabsf(t) > 16777216.0f", "ties to even", "min_key 0xffffffff and max_key 0",
                "below + above + sum(counts row) == n", "n_labels * bins at most 2^26", "field and labels being one container",
                "a NaN\n * keeps its payload", "0x7fc00000") if header == "f3d.h" else
               ("exactly in unsigned __int128", "(m - 1) / 20, (m - 1) / 2 and (m - 1) - (m - 1) / 20", "ldexp(sqrt(vq), -shift)",
                "24 - e clamped to -100 .. 100"))
    for needle in needles:
        assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    assert len(f3d._label_field_entry().argtypes) == 13 and len(f3d._paint_entry().argtypes) == 7
    field, labels = np.zeros((3, 4, 5), F32), np.ones((3, 4, 5), np.int64)
    for kw, match in ((dict(bins=257), "bins"), (dict(bins=-1), "bins"), (dict(bins=1.5), "bins"), (dict(shift=101), "shift"),
                      (dict(shift=0.5), "shift"), (dict(bins=4, range=(1.0, 1.0)), "range"), (dict(bins=4, range=(0.0, np.inf)), "range"),
                      (dict(n_labels=0), "n_labels"), (dict(n_labels=(1 << 22) + 1), "n_labels"), (dict(n_labels=1 << 20, bins=128), "2\\^26")):
        with pytest.raises(ValueError, match=match):
            f3d.label_field_sums(field, labels, **kw)
    with pytest.raises(ValueError, match="integers"):
        f3d.label_field_sums(field, field)
    with pytest.raises(ValueError, match="shape"):
        f3d.label_field_stats(field[:, :, :-1], labels)
    with pytest.raises(ValueError, match="non-empty"):
        f3d.label_field_sums(np.zeros((0, 4, 5), F32), np.ones((0, 4, 5), np.int32), n_labels=1)
    with pytest.raises(ValueError, match="LabelFieldSums"):
        f3d.solve_label_field(np.zeros(2, ref.SUMS_DTYPE))
    with pytest.raises(ValueError, match="one-dimensional"):
        f3d.paint_labels(np.zeros((2, 2), F32), labels)
    with pytest.raises(ValueError, match="integers"):
        f3d.paint_labels(np.zeros(2, F32), field)
    host = f3d.host()
    rows, out = (f3d.LabelFieldSumsRow * 1)(), (f3d.LabelFieldStat * 1)()
    counts = (C.c_uint * 4)()
    for args in ((None, None, 1, 0, 0, 0, 0, 1, out, None), (rows, None, 1, 0, 0, 0, 0, 1, None, None), (rows, None, 1, 101, 0, 0, 0, 1, out, None),
                 (rows, None, 1, 0, 0, 1, 4, 1, out, None), (rows, counts, 1, 0, 0, 1, 0, 1, out, None), (rows, counts, 1, 0, 1, 1, 4, 1, out, None),
                 (rows, counts, 1, 0, 0, 1, 257, 1, out, None)):
        assert host.f3d_label_field_solve(*args) != 0 and b"f3d_label_field_solve" in host.f3d_host_last_error()
    assert host.f3d_flow_label_field_compute(None, 0, 1, 0, None, 0, 1, out, None, None, None) != 0
    assert b"f3d_flow_label_field_compute" in host.f3d_host_last_error()
    assert host.f3d_flow_labels_paint(None, None, 1, None) != 0 and b"f3d_flow_labels_paint" in host.f3d_host_last_error()
    assert hasattr(f3d.OpticalFlow, "label_field") and hasattr(f3d.OpticalFlow, "paint_labels")


def test_the_automatic_shift(f3d):
    for lo, hi, finite in ((0.0, 65535.0, 9), (-0.07, 0.02, 9), (0.0, 0.0, 9), (1.0, 2.0, 0), (-3e38, 1.0, 9), (0.0, 1e-40, 9), (np.inf, -np.inf, 0),
                           (-1.0, 0.5, 9), (1.0, 16777216.0, 9), (0.0, 16777215.0, 9), (3.0, 3.0, 1)):
        assert f3d.label_field_shift(lo, hi, finite) == ref.shift_of(lo, hi, finite), (lo, hi, finite)
    # a uint16 grey value is kept exactly: q is the value times 2^8, no tie, nothing out of range
    grey = np.random.default_rng(2).integers(0, 65536, (4, 5, 6)).astype(np.uint16)
    grey[0, 0, 0] = 65535
    shift = f3d.label_field_shift(0, 65535)
    assert shift == 8
    rows, _, info = ref.label_field_sums(grey.astype(F32), np.ones(grey.shape, np.int32), 1, shift)
    assert info["used"] == grey.size and int(rows["iq"][0]) == int(grey.astype(np.int64).sum()) << 8
    assert (int(rows["iqq_hi"][0]) << 32) + int(rows["iqq_lo"][0]) == int((grey.astype(np.int64) ** 2).sum()) << 16
    # a strain-like field: the largest magnitude lands in [2^23, 2^24) quanta, so the quantum is below 2^-23 of it
    strain = np.random.default_rng(4).normal(0.0, 0.01, (4, 5, 6)).astype(F32)
    lo, hi, found = ref.href.value_range(strain)
    shift = f3d.label_field_shift(lo, hi, found["finite"])
    largest = max(abs(float(lo)), abs(float(hi)))
    assert 2 ** 23 <= largest * 2.0 ** shift < 2 ** 24
    _, _, info = ref.label_field_sums(strain, np.ones(strain.shape, np.int32), 1, shift)
    assert info["out_of_range"] == 0 and info["used"] == strain.size


CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    labels = np.ones((D, H, W), np.int32); labels[:, :, 10:] = 2
    field = np.zeros((D, H, W), np.float32)
    h = pkg.host()
    out, info = (pkg.LabelFieldStat * 2)(), pkg.LabelFieldInfo()
    assert h.f3d_flow_label_field_compute(flow._h, 0, 2, 0, None, 0, 1, out, None, info, None) != 0
    assert b"f3d_label_field_sums" in h.f3d_host_last_error(), h.f3d_host_last_error()
    paint = np.zeros(2, np.float32)
    assert h.f3d_flow_labels_paint(flow._h, paint.ctypes.data_as(pkg._fp), 2, field.ctypes.data_as(pkg._fp)) != 0
    assert b"f3d_paint_labels" in h.f3d_host_last_error(), h.f3d_host_last_error()
    for call, name in ((lambda: pkg.label_field_sums(field, labels, shift=0), "f3d_label_field_sums"),
                       (lambda: pkg.label_field_stats(field, labels, shift=0), "f3d_label_field_sums"),
                       (lambda: pkg.paint_labels(paint, labels), "f3d_paint_labels"), (lambda: flow.paint_labels(paint), "f3d_paint_labels")):
        try:
            call(); raise SystemExit("a call succeeded without " + name)
        except pkg.F3dError as e:
            assert name in str(e), str(e)
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_label_field_sums nor f3d_paint_labels: libf3d_host.so built against it must still load
    (RTLD_NOW), and the calls must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_label_field_sums" not in names and "f3d_paint_labels" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("case,needle", [
    ("no-labels", "--label-stats needs --labels FILE or --segment"), ("bins-alone", "need --label-stats"), ("paint-alone", "need --label-stats"),
    ("partial", "--label-stats needs the resident"), ("concurrent", "--label-stats needs the resident"), ("unknown", "is not one of"),
    ("twice", "given twice"), ("bins-257", "B must be 0 .. 256"), ("bins-negative", "B must be 0 .. 256"),
    ("vol", "needs --strain vol"), ("eq", "needs --strain eq"), ("eq-other", "needs --strain eq"), ("gmax", "needs --principal shear"),
    ("gmax-other", "needs --principal shear"), ("angle", "needs --rotation angle"), ("zncc", "needs --match zncc"), ("rmsd", "needs --match rmsd"),
    ("wvol", "needs --window-strain vol"), ("weq", "needs --window-strain eq"), ("zncc-cumulative", "cannot be combined with --cumulative"),
    ("rmsd-cumulative", "cannot be combined with --cumulative"), ("three-frames", "needs --cumulative")])
def test_flow3d_label_stats_argument_errors(tmp_path, case, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    good = str(tmp_path / "labels.raw")
    np.ones(64, np.int32).tofile(good)
    lab = ["--labels", good]
    extra = {"no-labels": ["--label-stats", "grey"], "bins-alone": lab + ["--label-shape", "--label-stats-bins", "8"],
             "paint-alone": lab + ["--label-shape", "--label-stats-paint"], "partial": lab + ["--label-stats", "grey", "--partial"],
             "concurrent": lab + ["--label-stats", "grey", "--concurrent", "2"], "unknown": lab + ["--label-stats", "grey,exx"],
             "twice": lab + ["--label-stats", "grey,grey"], "bins-257": lab + ["--label-stats", "grey", "--label-stats-bins", "257"],
             "bins-negative": lab + ["--label-stats", "grey", "--label-stats-bins", "-1"], "vol": lab + ["--label-stats", "vol"],
             "eq": lab + ["--label-stats", "grey,eq"], "eq-other": lab + ["--label-stats", "eq", "--strain", "vol,e"],
             "gmax": lab + ["--label-stats", "gmax"], "gmax-other": lab + ["--label-stats", "gmax", "--principal", "val"],
             "angle": lab + ["--label-stats", "angle", "--rotation", "vector"], "zncc": lab + ["--label-stats", "zncc", "--match", "rmsd"],
             "rmsd": lab + ["--label-stats", "rmsd"], "wvol": lab + ["--label-stats", "wvol", "--window-strain", "eq"],
             "weq": lab + ["--label-stats", "weq"], "zncc-cumulative": lab + ["--label-stats", "zncc", "--match", "zncc", "--cumulative"],
             "rmsd-cumulative": lab + ["--label-stats", "rmsd", "--match", "rmsd", "--cumulative"],
             "three-frames": lab + ["--label-stats", "eq", "--strain", "eq"]}[case]
    frames = paths if case == "three-frames" else paths[:2]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *frames, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "--label-stats grey,vol,eq,gmax,angle,zncc,rmsd,wvol,weq" in run.stdout
    assert "[(--labels FILE | --segment ...) --label-shape]" in run.stdout                          # the earlier usage text is all there
    assert "3D optical flow" not in run.stdout                                                   # before any device is touched
    assert not any("labelstats" in n or "flow-" in n for n in os.listdir(tmp_path))
