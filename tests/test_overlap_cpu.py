"""The overlap of two label volumes and the tracks of their bodies without a GPU: the numpy restatement (tests/overlap_ref.py) against
a plain loop over the voxels and against cases whose rows are known; the float32 rounding of the landing voxel; the host solve
(f3d_overlap_solve) bit for bit against the restatement and on bodies that split, merge, vanish, appear and leave; the solve under
AddressSanitizer and UBSan in a stand-alone program; the struct layouts; the binding's argument checks; the message of a device
library without f3d_label_overlap; and the refusals of bin/flow3d --track.

Bounds.  Every count and sum is an exact integer, and every double of the solve is one conversion and one division of exact integers
in a stated order, so the host library and the restatement agree bit for bit: the comparison is of bytes."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import overlap_ref as ref
from label_motion_ref import voronoi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
HOST = os.path.join(ROOT, "cuda-flow3d_amd", "host")
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flow", [False, True], ids=["identity", "flow"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 2), (2, 1, 1), (2, 2, 2), (1, 5, 4), (3, 4, 5), (6, 5, 7)], ids=str)
def test_the_restatement_against_a_loop_over_the_voxels(shape, flow):
    rng = np.random.default_rng(sum(shape) + flow)
    a = rng.integers(-1, 5, shape).astype(np.int32)                    # background, foreign on both sides (-1 and 4), three bodies
    b = rng.integers(-1, 6, shape).astype(np.int32)
    a[rng.random(shape) < 0.05] = np.iinfo(np.int32).min
    d = (None, None, None)
    if flow:
        d = tuple(rng.choice(np.array([0, 0, 0.5, -0.5, 1, -1, 1.49, 2.5, -3, np.nan, np.inf], F32), size=shape) for _ in range(3))
    fast, info = ref.label_overlap(a, 3, b, 4, *d)
    slow, info_slow = ref.label_overlap_loops(a, 3, b, 4, *d)
    assert ref.as_table(fast) == slow and info == info_slow
    assert sum(info[c] for c in ref.CLASSES) == np.prod(shape) and int(fast["n"].sum()) == info["lost_body"] + info["overlap"]
    keys = list(zip(fast["a"].tolist(), fast["b"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and (0, 0) not in keys and (0, -1) not in keys
    assert (fast["cb2"][fast["b"] == -1] == 0).all()
    assert ref.rows_of(slow).tobytes() == fast.tobytes()


def test_the_identity_of_a_volume_with_itself_is_the_diagonal():
    lab = voronoi((9, 10, 11), 12, seed=3)
    lab[lab == 5] = 0
    rows, info = ref.label_overlap(lab, 12, lab, 12)
    count = np.bincount(lab.ravel(), minlength=13)
    present = [l for l in range(1, 13) if count[l]]
    assert rows["a"].tolist() == rows["b"].tolist() == present and rows["n"].tolist() == [count[l] for l in present]
    assert (rows["ca2"] == rows["cb2"]).all() and info["background"] == count[0] and info["overlap"] == lab.size - count[0]
    zero = np.zeros(lab.shape, F32)
    again, info_zero = ref.label_overlap(lab, 12, lab, 12, zero, -zero, zero)      # a zero displacement, of either sign
    assert again.tobytes() == rows.tobytes() and info_zero == info


def test_an_integer_shift_of_a_block():
    d, h, w = 8, 9, 10
    a = np.zeros((d, h, w), np.int32)
    a[2:6, 3:7, 4:9] = 1                                               # x 4 .. 8, y 3 .. 6, z 2 .. 5: 5 x 4 x 4 = 80 voxels
    sx, sy, sz = 3, -2, 1
    b = np.zeros_like(a)
    b[3:7, 1:5, 7:10] = 2                                              # where it lands, cut at x = 9
    u, v, ww = (np.full(a.shape, s, F32) for s in (sx, sy, sz))
    rows, info = ref.label_overlap(a, 1, b, 2, u, v, ww)
    table = ref.as_table(rows)
    assert sorted(table) == [(1, -1), (1, 2)]
    assert table[(1, 2)][0] == 3 * 4 * 4 and table[(1, -1)][0] == 2 * 4 * 4     # x = 7, 8 leave through the +x face
    n, ca2, cb2 = table[(1, 2)]
    assert [(q - p) / (2 * n) for p, q in zip(ca2, cb2)] == [sx, sy, sz]
    assert ca2 == [sum(2 * x - (w - 1) for x in (4, 5, 6)) * 16, sum(2 * y - (h - 1) for y in range(3, 7)) * 12,
                   sum(2 * z - (d - 1) for z in range(2, 6)) * 12]
    assert table[(1, -1)][2] == [0, 0, 0] and table[(1, -1)][1][0] == (2 * 7 - 9 + 2 * 8 - 9) * 16
    # the background: lost where it leaves the box, else on background (nothing of B is left unreached here)
    assert info["lost_body"] == 32 and info["overlap"] == 48 and info["foreign_a"] == info["foreign_b"] == 0
    assert info["lost_background"] + info["background"] == a.size - 80
    ta, tb, map_b, summary = ref.solve(rows, 1, 2, 0.1)
    assert ta["shift"][0].tolist() == [sx, sy, sz] and ta["status"][0] == ref.MATCHED | ref.LEFT and ta["n_lost"][0] == 32
    assert map_b.tolist() == [0, 1] and tb["status"].tolist() == [ref.EMPTY, ref.MATCHED] and summary["n_ids"] == 1


def test_the_float32_add_decides_the_landing_voxel():
    """p + 0.5f on the tie goes up (floor of an exact k + 1); at the float below 0.5 the exact sum x + t + 0.5 lies below x + 1, but
    the float32 adds round it to x + 1 (at x = 0 the sum 1 - 2^-25 is a tie that goes to the even 1.0f; from x = 1 on x + t itself
    already rounds to x + 0.5): the voxel lands one further than real arithmetic says, and the restatement and the kernel must agree"""
    below = np.nextafter(F32(0.5), F32(0))
    w = 12
    a = np.ones((1, 1, w), np.int32)
    b = np.arange(1, w + 1, dtype=np.int32).reshape(1, 1, w)
    zero = np.zeros((1, 1, w), F32)
    for t, landing in ((F32(0.5), [x + 1 for x in range(w)]), (below, [x + 1 for x in range(w)]),
                       (-below, list(range(w))), (F32(-0.5), list(range(w)))):
        u = np.full((1, 1, w), t, F32)
        inside, (yx, _, _) = ref.landing((1, 1, w), u, zero, zero)
        keep = inside[0, 0]
        assert yx[0, 0][keep].tolist() == [l for l, k in zip(landing, keep) if k], float(t)
        rows, info = ref.label_overlap(a, 1, b, w, u, zero, zero)
        assert sorted(ref.as_table(rows)) == sorted(ref.label_overlap_loops(a, 1, b, w, u, zero, zero)[0])
    # x = 0 with t = -0.5 leaves the box (p < 0); with t = +0.5 the last voxel does (p > w - 1)
    assert ref.label_overlap(a, 1, b, w, np.full((1, 1, w), -0.5, F32), zero, zero)[1]["lost_body"] == 1
    assert ref.label_overlap(a, 1, b, w, np.full((1, 1, w), 0.5, F32), zero, zero)[1]["lost_body"] == 1
    assert F32(1) + below + F32(0.5) == F32(2) and below + F32(0.5) == F32(1) and float(below) + 0.5 < 1.0


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------

def scene():
    """A: 1 breaks in two, 2 and 3 merge, 4 vanishes, 5 leaves through +x, 6 has no voxel.  B: 4 appears, 5 has no voxel."""
    a = np.zeros((6, 20, 40), np.int32)
    b = np.zeros_like(a)
    a[1:5, 1:5, 1:11] = 1
    b[1:5, 1:5, 1:7], b[1:5, 1:5, 7:11] = 1, 2                           # 96 and 64 of 160 voxels
    a[1:5, 7:11, 1:6], a[1:5, 7:11, 6:10] = 2, 3                          # 80 and 64
    b[1:5, 7:11, 1:10] = 3
    a[1:5, 13:17, 1:5] = 4
    a[1:5, 13:17, 30:40] = 5
    b[1:5, 13:17, 10:14] = 4
    u = np.zeros(a.shape, F32)
    u[a == 5] = 7.0                                                       # x 30 .. 39 + 7: x >= 33 leaves
    return a, 6, b, 5, u


def test_split_merge_vanish_appear_leave_and_the_new_numbers():
    a, n_a, b, n_b, u = scene()
    zero = np.zeros(a.shape, F32)
    rows, info = ref.label_overlap(a, n_a, b, n_b, u, zero, zero)
    ta, tb, map_b, summary = ref.solve(rows, n_a, n_b, 0.1)
    assert ta["status"].tolist() == [ref.MATCHED | ref.SPLIT, ref.MATCHED, 0, ref.VANISHED, ref.VANISHED | ref.LEFT, ref.EMPTY]
    assert tb["status"].tolist() == [ref.MATCHED, 0, ref.MATCHED | ref.MERGED, ref.APPEARED, ref.EMPTY]
    assert map_b.tolist() == [1, 7, 2, 8, 0]                             # the larger fragment keeps the number, the others are new
    assert summary == dict(matched=2, split=1, merged=1, vanished=2, appeared=1, left=1, n_ids=8)
    assert ta["n"].tolist() == [160, 80, 64, 64, 160, 0] and ta["n_best"].tolist() == [96, 80, 64, 0, 0, 0]
    assert ta["n_lost"][4] == 7 * 16 and ta["n_background"][4] == 3 * 16 and ta["n_background"][3] == 64
    assert ta["fraction"][:5].tolist() == [0.6, 1.0, 1.0, 0.0, 0.0] and np.isnan(ta["fraction"][5]) and np.isnan(ta["shift"][3]).all()
    assert ta["iou"][:5].tolist() == [96 / 160, 80 / 144, 64 / 144, 0.0, 0.0] and (ta["shift"][:3] == 0).all()
    assert tb["m"].tolist() == [96, 64, 144, 64, 0] and tb["n_unreached"].tolist() == [0, 0, 0, 64, 0] and tb["best_a"].tolist() == [1, 1, 2, 0, 0]
    out, foreign = ref.relabel(b, map_b)
    assert foreign == 0 and sorted(np.unique(out).tolist()) == [0, 1, 2, 7, 8] and (out[b == 2] == 7).all() and (out[b == 3] == 2).all()
    # min_fraction decides what counts: at 0.5 the smaller fragment is no target and body 3 no source
    ta, tb, _, summary = ref.solve(rows, n_a, n_b, 0.5)
    assert ta["status"][0] == ref.MATCHED and tb["status"][2] == ref.MATCHED and summary["split"] == summary["merged"] == 0
    assert ref.solve(rows[::-1], n_a, n_b, 0.1)[2].tolist() == [1, 7, 2, 8, 0]   # rows in any order


def as_c(f3d, rows):
    out = (f3d.Overlap * max(len(rows), 1))()
    flat = np.ascontiguousarray(rows)                                  # held until the bytes are across
    if len(rows):
        C.memmove(out, flat.ctypes.data, flat.nbytes)
    return f3d.Overlaps(out, len(rows), None)


@pytest.mark.parametrize("min_fraction", [0.1, 1.0 / 3.0, 0.5, 1.0])
def test_the_host_solve_equals_the_restatement_bit_for_bit(f3d, min_fraction):
    a, n_a, b, n_b, u = scene()
    cases = [(a, n_a, b, n_b, (u, np.zeros(a.shape, F32), np.zeros(a.shape, F32)))]
    shape = (12, 14, 16)
    rng = np.random.default_rng(11)
    a, b = voronoi(shape, 30, seed=1), voronoi(shape, 25, seed=2)
    a[rng.random(shape) < 0.2] = 0
    b[rng.random(shape) < 0.2] = 0
    cases.append((a, 33, b, 28, tuple(rng.uniform(-3, 3, shape).astype(F32) for _ in range(3))))   # spare numbers on both sides
    for a, n_a, b, n_b, d in cases:
        rows, _ = ref.label_overlap(a, n_a, b, n_b, *d)
        want_a, want_b, want_map, want_summary = ref.solve(rows, n_a, n_b, min_fraction)
        got = f3d.solve_overlaps(as_c(f3d, rows), n_a, n_b, min_fraction)
        assert got.a.tobytes() == want_a.tobytes() and got.b.tobytes() == want_b.tobytes()
        assert got.map_b.tobytes() == want_map.tobytes() and got.summary == want_summary
        turned = f3d.solve_overlaps(as_c(f3d, rows[::-1]), n_a, n_b, min_fraction)
        assert turned.a.tobytes() == want_a.tobytes() and turned.map_b.tobytes() == want_map.tobytes()
        table = got.as_table()
        assert len(table) == n_a + n_b and table[0]["side"] == "a" and table[-1]["side"] == "b" and "new_label" in table[-1]
    empty = f3d.solve_overlaps(as_c(f3d, rows[:0]), 2, 3, 0.1)
    assert empty.a["status"].tolist() == [ref.EMPTY] * 2 and empty.map_b.tolist() == [0, 0, 0] and empty.summary["n_ids"] == 2


def test_the_solve_under_the_sanitizers(tmp_path):
    """host/label_track.cpp and tests/overlap_solve_main.cpp built into a program of their own with AddressSanitizer and UBSan"""
    exe = tmp_path / "overlap_solve"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(HOST, "label_track.cpp"), os.path.join(ROOT, "tests", "overlap_solve_main.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-2000:], run.stderr[-3000:])


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_the_header(f3d, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(textwrap.dedent('''
        #include <stddef.h>
        #include <stdio.h>
        #include "f3d_host.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu\\n", sizeof(struct f3d_overlap), offsetof(struct f3d_overlap, b), offsetof(struct f3d_overlap, n),
                 offsetof(struct f3d_overlap, ca2), offsetof(struct f3d_overlap, cb2));
          printf("%zu %zu %zu %zu\\n", sizeof(f3d_overlap_info), offsetof(f3d_overlap_info, overlap), offsetof(f3d_overlap_info, n_pairs),
                 offsetof(f3d_overlap_info, complete));
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(f3d_track_a), offsetof(f3d_track_a, n_lost),
                 offsetof(f3d_track_a, n_background), offsetof(f3d_track_a, n_best), offsetof(f3d_track_a, best_b),
                 offsetof(f3d_track_a, n_targets), offsetof(f3d_track_a, fraction), offsetof(f3d_track_a, shift), offsetof(f3d_track_a, iou),
                 offsetof(f3d_track_a, status));
          printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(f3d_track_b), offsetof(f3d_track_b, n_unreached), offsetof(f3d_track_b, n_best),
                 offsetof(f3d_track_b, best_a), offsetof(f3d_track_b, n_sources), offsetof(f3d_track_b, status));
          printf("%zu %zu\\n", sizeof(f3d_track_summary), offsetof(f3d_track_summary, n_ids));
          printf("%u %u %u %u %u %u %u\\n", F3D_TRACK_EMPTY, F3D_TRACK_MATCHED, F3D_TRACK_SPLIT, F3D_TRACK_VANISHED, F3D_TRACK_LEFT,
                 F3D_TRACK_MERGED, F3D_TRACK_APPEARED);
          return 0;
        }'''))
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    lines = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    O, I, A, B, S = f3d.Overlap, f3d.OverlapInfo, f3d.TrackA, f3d.TrackB, f3d.TrackSummary
    assert lines[0] == [C.sizeof(O), O.b.offset, O.n.offset, O.ca2.offset, O.cb2.offset] == [64, 4, 8, 16, 40]
    assert lines[1] == [C.sizeof(I), I.overlap.offset, I.n_pairs.offset, I.complete.offset] == [72, 40, 56, 64]
    a_fields = ("n_lost", "n_background", "n_best", "best_b", "n_targets", "fraction", "shift", "iou", "status")
    assert lines[2] == [C.sizeof(A)] + [getattr(A, n).offset for n in a_fields] == [88, 8, 16, 24, 32, 36, 40, 48, 72, 80]
    b_fields = ("n_unreached", "n_best", "best_a", "n_sources", "status")
    assert lines[3] == [C.sizeof(B)] + [getattr(B, n).offset for n in b_fields] == [40, 8, 16, 24, 28, 32]
    assert lines[4] == [C.sizeof(S), S.n_ids.offset] == [56, 48]
    assert lines[5] == [ref.EMPTY, ref.MATCHED, ref.SPLIT, ref.VANISHED, ref.LEFT, ref.MERGED, ref.APPEARED]
    assert lines[5] == [f3d.TRACK_STATUS[k] for k in ("empty", "matched", "split", "vanished", "left", "merged", "appeared")]
    assert f3d._OVERLAP_DTYPE == ref.ROWS_DTYPE and f3d._TRACK_A_DTYPE == ref.TRACK_A_DTYPE and f3d._TRACK_B_DTYPE == ref.TRACK_B_DTYPE
    for dtype, struct in ((ref.ROWS_DTYPE, O), (ref.TRACK_A_DTYPE, A), (ref.TRACK_B_DTYPE, B)):
        assert dtype.itemsize == C.sizeof(struct)
        for name in dtype.names:
            if name != "pad":
                assert dtype.fields[name][1] == getattr(struct, name).offset, name


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_label_overlap", "f3d_relabel_labels"]),
                                              ("f3d_host.h", "host", ["f3d_overlap_solve", "f3d_flow_labels_b_upload", "f3d_flow_labels_b_segment",
                                                                      "f3d_flow_overlap_compute", "f3d_flow_overlap_end",
                                                                      "f3d_flow_labels_b_relabel", "f3d_flow_labels_b_download"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    if header == "f3d.h":                                      # the definition stands in the header in full
        for needle in ("foreign_a", "lost_background", "min(N_c - 1, (int)floorf(p_c + 0.5f))", "the key (a, -1)", "2 x_j - (N_j - 1)",
                       "every sum below 2^49", "2 * capacity slots of 64 B", "(a, -1) leads the rows of a", "NOTHING is written to out",
                       "labels_a and\n * labels_b being one container", "Container padding is never read", "out may be labels itself"):
            assert needle in text, needle
    else:
        for needle in ("(double)p >= min_fraction * (double)q", "ties to the smallest b", "(double)(cb2_j - ca2_j) / (2.0 * (double)n_best)",
                       "not the voxel count of b in its own volume", "(double)n_best / (double)(n + m_(best_b) - n_best)",
                       "n_a + 1, n_a + 2, ... in ascending b", "the resident frame 1"):
            assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    assert len(f3d._overlap_entry().argtypes) == 13 and len(f3d._relabel_entry().argtypes) == 8
    good = np.ones((3, 4, 5), np.int64)
    zero = np.zeros((3, 4, 5), F32)
    with pytest.raises(ValueError, match="integers"):
        f3d.label_overlap(zero, good)
    with pytest.raises(ValueError, match="integers"):
        f3d.label_overlap(good, good[0])
    with pytest.raises(ValueError, match="all three"):
        f3d.label_overlap(good, good, zero, None, zero)
    with pytest.raises(ValueError, match="n_labels"):
        f3d.label_overlap(good, good * 0)
    with pytest.raises(ValueError, match="n_labels"):
        f3d.label_overlap(good, good, n_a=(1 << 22) + 1)
    with pytest.raises(ValueError, match="capacity"):
        f3d.label_overlap(good, good, capacity=0)
    with pytest.raises(ValueError, match="capacity"):
        f3d.label_overlap(good, good, capacity=(1 << 24) + 1)
    with pytest.raises(ValueError, match="one-dimensional"):
        f3d.relabel_labels(good, np.ones((2, 2), np.int32))
    with pytest.raises(ValueError, match="one-dimensional"):
        f3d.relabel_labels(good, np.ones(3, F32))
    with pytest.raises(ValueError, match="entries of mapping"):
        f3d.relabel_labels(good, [1, -1])
    with pytest.raises(ValueError, match="n_labels"):
        f3d.relabel_labels(good, np.zeros(0, np.int32))
    none = as_c(f3d, np.zeros(0, ref.ROWS_DTYPE))
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_fraction"):
            f3d.solve_overlaps(none, 1, 1, bad)
    with pytest.raises(ValueError, match="n_a and n_b"):
        f3d.solve_overlaps(none, 0, 1)
    host = f3d.host()
    rows, a, b, m = (f3d.Overlap * 1)(), (f3d.TrackA * 2)(), (f3d.TrackB * 2)(), (C.c_int * 2)()
    for args in ((None, 1, 2, 2, 0.1, a, b, m, None), (rows, 1, 2, 2, 0.1, None, b, m, None), (rows, 1, 2, 2, 0.1, a, None, m, None),
                 (rows, 1, 2, 2, 0.1, a, b, None, None), (rows, 0, 0, 2, 0.1, a, b, m, None), (rows, 0, 2, 2, 2.0, a, b, m, None)):
        assert host.f3d_overlap_solve(*args) != 0 and b"f3d_overlap_solve" in host.f3d_host_last_error(), args
    rows[0].a, rows[0].b, rows[0].n = 3, 1, 5                           # a key outside 0 .. n_a
    assert host.f3d_overlap_solve(rows, 1, 2, 2, 0.1, a, b, m, None) != 0 and b"(3, 1)" in host.f3d_host_last_error()
    for name, args in (("f3d_flow_labels_b_upload", (None, m)), ("f3d_flow_labels_b_download", (None, m)),
                       ("f3d_flow_labels_b_relabel", (None, m, 2)), ("f3d_flow_overlap_end", (None,)),
                       ("f3d_flow_overlap_compute", (None, 0, 1, 1, None, None, None)),
                       ("f3d_flow_labels_b_segment", (None, 0, 0.0, 1.0, 0, 1, None, None, None))):
        assert getattr(host, name)(*args) != 0 and name.encode() in host.f3d_host_last_error(), name
    for method in ("segment_next", "track", "track_end"):
        assert hasattr(f3d.OpticalFlow, method)
    table = f3d.Overlaps((f3d.Overlap * 1)(), 0, None)
    assert len(table) == 0 and table.matrix() == {} and table.as_table() == [] and table.matrix(2, 3).shape == (3, 5)


CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    labels = np.ones((D, H, W), np.int32); labels[:, :, 10:] = 2
    calls = {"f3d_label_overlap": [lambda: pkg.label_overlap(labels, labels), lambda: pkg.track_labels(labels, labels),
                                   lambda: flow.track(labels, n_a=2, relabel=False)],
             "f3d_relabel_labels": [lambda: pkg.relabel_labels(labels, [2, 1])]}
    for entry, tries in calls.items():
        for call in tries:
            try:
                call(); raise SystemExit("a call succeeded without " + entry)
            except pkg.F3dError as e:
                assert entry in str(e), str(e)
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_label_overlap nor f3d_relabel_labels: libf3d_host.so built against it must still load
    (RTLD_NOW), and the calls must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_label_overlap" not in names and "f3d_relabel_labels" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("case,needle", [("no-segment", "--track follows the bodies --segment makes"),
                                         ("fraction-alone", "--track-min-fraction needs --track"),
                                         ("fraction-zero", "F must be in (0, 1]"), ("fraction-large", "F must be in (0, 1]"),
                                         ("fraction-nan", "F must be in (0, 1]"), ("fraction-word", "F must be in (0, 1]"),
                                         ("three-frames", "--track of more than two frames needs --cumulative"),
                                         ("partial", "--track needs the resident driver"), ("concurrent", "--track needs the resident driver")])
def test_flow3d_track_argument_errors(tmp_path, case, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3 if case == "three-frames" else 2):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    seg = ["--segment", "0.5:"]
    extra = {"no-segment": ["--track"], "fraction-alone": seg + ["--track-min-fraction", "0.2"],
             "fraction-zero": seg + ["--track", "--track-min-fraction", "0"], "fraction-large": seg + ["--track", "--track-min-fraction", "1.01"],
             "fraction-nan": seg + ["--track", "--track-min-fraction", "nan"], "fraction-word": seg + ["--track", "--track-min-fraction", "half"],
             "three-frames": seg + ["--track"], "partial": seg + ["--track", "--partial"],
             "concurrent": seg + ["--track", "--concurrent", "2"]}[case]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "--track [--track-min-fraction F]" in run.stdout and "an Otsu cut is not taken again per frame" in run.stdout
    assert not [n for n in os.listdir(tmp_path) if n.startswith("o")]   # nothing was written
