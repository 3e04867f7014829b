"""Statistics of a scalar field per labelled body on the GPU: f3d_label_field_sums against its numpy restatement
(tests/label_field_ref.py), never against itself, every word of every row, every count and the info bit for bit; three independent
kernels as cross-checks (f3d_histogram, f3d_label_shape_sums, f3d_value_range); the refusals; f3d_paint_labels; label_field_stats and
paint_labels from anywhere, OpticalFlow.label_field on a held flow; and bin/flow3d --label-stats in a two-frame run whose other outputs
stay byte for byte the same.

Bounds.  Every word is an exact integer of the input: equality, whatever the schedule, and two calls give the same bytes.  The solve is
the host's, held to the restatement bit for bit in tests/test_label_field_cpu.py.

Shapes.  The kernel's tile is 64 x 4 x 32 and a lane loads four planes at a time: 64x4x32 is exactly one tile, 65x5x33 one voxel more
along every axis, 130x9x70 has three tiles along x and z and a last load group of two planes; 1x1x1, 2x2x2 and 3x70x2 are thinner than
a load group.  The label table in LDS has 128 slots: the 1000 random labels overflow it in every full tile, so runs go straight to the
global rows, and with 64 or 256 bins their (label, bin) pairs overflow the 1024 slots of the second table too.

Padding.  The box lies in the corner of containers three columns, two rows and a plane larger, whose float padding is NaN and whose label
padding carries the valid label 1: a kernel that reads padding counts NaN voxels and voxels of label 1 that are not there.

Host memory and the module's name.  The name makes it sort behind tests/test_gpu_pipeline.py, whose page-locked test is sensitive to what
ran in the process before it (LABBOOK.md).  For the same reason the restatement runs in a child interpreter, once for all cases, the
tests read its volumes, containers and rows as read-only file mappings, and nothing in this module page-locks host memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import label_field_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SENTINEL = 0x7F
SHAPES = [(1, 1, 1), (2, 2, 2), (64, 4, 32), (65, 5, 33), (3, 70, 2), (130, 9, 70)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) and isinstance(s[0], int) else "-".join(s) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(dims, (layout, kind)) -> (arrays, settings): every case computed once, by a child interpreter, and read as read-only file
    mappings (label_field_ref.in_child says why)"""
    keys = [(dims, case) for dims in SHAPES for case in ref.CASES]
    made = ref.in_child([[list(dims), *case] for dims, case in keys], str(tmp_path_factory.mktemp("label_field_cases")))
    return dict(zip(keys, made))


def device_sums(f3d, arrays, dims, n_labels, shift, lo, hi, bins, calls=1, info=True):
    """f3d_label_field_sums on the box `dims` in the corner of the case's containers: (rows as a structured array, counts or None, info
    dict) per call; rows and counts are filled with the sentinel byte before every call"""
    w, h, d = dims
    fn = f3d._label_field_entry()
    dc, hc, wc = arrays["label_box"].shape
    box = f3d.Containers(wc, hc, dc)
    try:
        fl = box.new(arrays["field_box"])
        pl = box.new(arrays["label_box"].view(F32))
        box.set_current()
        out = []
        for _ in range(calls):
            rows, counted = (f3d.LabelFieldSumsRow * n_labels)(), f3d.LabelFieldInfo()
            C.memset(rows, SENTINEL, C.sizeof(rows))
            counts = np.full((n_labels, bins), 0x7F7F7F7F, np.uint32) if bins else None
            f3d.check(fn(fl, pl, n_labels, shift, lo, hi, bins, w, h, d, rows, counts.ctypes.data_as(C.POINTER(C.c_uint)) if bins else None,
                         C.byref(counted) if info else None), "f3d_label_field_sums")
            out.append((np.frombuffer(rows, ref.SUMS_DTYPE), counts, counted.as_dict()))
    finally:
        box.free()
    return out if calls > 1 else out[0]


def check_rows(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() == want.tobytes():
        return
    for name in ref.SUMS_DTYPE.names:                                    # say which word of which label differs
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, (name, "label", int(bad[0][0]) + 1, int(got[name][bad[0][0]]), int(want[name][bad[0][0]]))


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", ref.BINS)
@pytest.mark.parametrize("case", ref.CASES, ids=ids)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_sums_equal_the_restatement_bit_for_bit(f3d, cases, dims, case, bins):
    arrays, s = cases[dims, case]
    n_labels = s["n_labels"]
    (rows, counts, info), (rows2, counts2, info2) = device_sums(f3d, arrays, dims, n_labels, s["shift"], s["lo"], s["hi"], bins, calls=2)
    assert rows.tobytes() == rows2.tobytes() and info == info2           # two calls, identical bytes
    assert info == s["info"]
    check_rows(rows, np.asarray(arrays[f"rows_{bins}"]))
    w, h, d = dims
    assert sum(info.values()) == w * h * d and int(rows["n"].sum()) == info["used"]
    if bins:
        assert counts.tobytes() == counts2.tobytes()
        want = np.asarray(arrays[f"counts_{bins}"])
        bad = np.argwhere(counts != want)
        assert bad.size == 0, ("label", int(bad[0][0]) + 1, "bin", int(bad[0][1]), int(counts[tuple(bad[0])]), int(want[tuple(bad[0])]))
        assert np.array_equal(rows["below"] + rows["above"] + counts.sum(axis=1, dtype=np.uint64), rows["n"])
    else:
        assert not rows["below"].any() and not rows["above"].any()
    empty = rows["n"] == 0
    assert (rows["min_key"][empty] == 0xFFFFFFFF).all() and (rows["max_key"][empty] == 0).all() and not rows["iq"][empty].any()
    if w * h * d > 100:
        layout, kind = case
        if layout == "spare":
            assert empty[40:].all() and not empty[:40].all()             # the spare labels, and in a thin box some of the cells
        if layout == "outside":
            assert info["foreign"] > 0 and info["background"] > 0
        if kind in ("noise", "edges"):
            assert info["out_of_range"] > 0 and (info["nan"] > 0) == (kind == "noise")
        if kind == "constant":
            assert int(rows["min_key"][0]) == int(rows["max_key"][0]) and info["used"] == w * h * d
            if bins:
                assert int(counts[0, -1]) == w * h * d                    # s == hi lands in the last bin


def test_the_info_is_optional(f3d, cases):
    dims, case = (65, 5, 33), ("voronoi", "ramp")
    arrays, s = cases[dims, case]
    rows, counts, _ = device_sums(f3d, arrays, dims, s["n_labels"], s["shift"], s["lo"], s["hi"], 64, info=False)
    check_rows(rows, np.asarray(arrays["rows_64"]))
    assert np.array_equal(counts, arrays["counts_64"])


# ---- cross-checks against independent kernels -------------------------------------------------------------------------------------------------

def test_one_label_everywhere_counts_as_the_histogram_does(f3d, cases):
    """every voxel between lo and hi takes part (|s| <= 1024 = 2^24 quanta), so the bins are f3d_histogram's; the voxels it counts below
    and above are this entry's, and those out of range"""
    dims, case = (130, 9, 70), ("one", "noise")
    arrays, s = cases[dims, case]
    rows, counts, info = device_sums(f3d, arrays, dims, 1, s["shift"], s["lo"], s["hi"], 256)
    hist = f3d.histogram(np.asarray(arrays["field"]), 256, range=(s["lo"], s["hi"]))
    assert counts[0].astype(np.uint64).tolist() == hist.counts.tolist() and hist.info["used"] == int(counts.sum()) > 10000
    assert hist.info["nan"] == info["nan"]
    assert hist.info["below"] + hist.info["above"] == int(rows["below"][0]) + int(rows["above"][0]) + info["out_of_range"]


def test_the_voxels_per_label_are_those_of_label_shape_sums(f3d, cases):
    dims, case = (65, 5, 33), ("voronoi", "integers")
    arrays, s = cases[dims, case]
    rows, _, info = device_sums(f3d, arrays, dims, s["n_labels"], s["shift"], s["lo"], s["hi"], 0)
    shapes, shape_info = f3d.label_shape_sums(np.asarray(arrays["labels"]), s["n_labels"])
    assert info["nan"] == info["out_of_range"] == 0 and info["used"] == shape_info["labelled"]
    assert rows["n"].tolist() == shapes["n"].tolist()


def test_the_extremes_of_a_label_are_those_of_value_range(f3d, cases):
    dims, case = (65, 5, 33), ("voronoi", "integers")
    arrays, s = cases[dims, case]
    rows, _, _ = device_sums(f3d, arrays, dims, s["n_labels"], s["shift"], s["lo"], s["hi"], 0)
    labels, field = np.asarray(arrays["labels"]), np.asarray(arrays["field"])
    for L in (1, 17, 40):
        lo, hi, found = f3d.value_range(field, mask=(labels == L))
        assert found["finite"] == int(rows["n"][L - 1]) > 0
        assert int(ref.href.key_of(lo).ravel()[0]) == int(rows["min_key"][L - 1]) and int(ref.href.key_of(hi).ravel()[0]) == int(rows["max_key"][L - 1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._label_field_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        lab = box.new(np.ones((8, 8, 8), np.int32).view(F32))
        fld = box.new(np.full((8, 8, 8), 1.5, F32))
        box.set_current()
        rows, info = (f3d.LabelFieldSumsRow * 2)(), f3d.LabelFieldInfo()
        counts = np.full(2 * 256, 0x7F7F7F7F, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint))
        C.memset(rows, SENTINEL, C.sizeof(rows))
        info.used = 55
        ip = C.byref(info)
        inf, nan = float("inf"), float("nan")
        #       field labels n shift lo hi bins w h d out counts info
        bad = [(0, lab, 2, 0, 0, 0, 0, 8, 8, 8, rows, None, ip), (fld, 0, 2, 0, 0, 0, 0, 8, 8, 8, rows, None, ip),
               (fld, lab, 2, 0, 0, 0, 0, 8, 8, 8, None, None, ip), (fld, fld, 2, 0, 0, 0, 0, 8, 8, 8, rows, None, ip),
               (fld, lab, 2, 101, 0, 0, 0, 8, 8, 8, rows, None, ip), (fld, lab, 2, -101, 0, 0, 0, 8, 8, 8, rows, None, ip),
               (fld, lab, 2, 0, 0, 1, 257, 8, 8, 8, rows, cp, ip), (fld, lab, 2, 0, 0, 1, 0, 8, 8, 8, rows, cp, ip),
               (fld, lab, 2, 0, 0, 1, 4, 8, 8, 8, rows, None, ip), (fld, lab, 2, 0, 1, 1, 4, 8, 8, 8, rows, cp, ip),
               (fld, lab, 2, 0, 2, 1, 4, 8, 8, 8, rows, cp, ip), (fld, lab, 2, 0, nan, 1, 4, 8, 8, 8, rows, cp, ip),
               (fld, lab, 2, 0, 0, inf, 4, 8, 8, 8, rows, cp, ip), (fld, lab, 2, 0, -3e38, 3e38, 4, 8, 8, 8, rows, cp, ip),
               (fld, lab, 0, 0, 0, 0, 0, 8, 8, 8, rows, None, ip), (fld, lab, (1 << 22) + 1, 0, 0, 0, 0, 8, 8, 8, rows, None, ip),
               (fld, lab, 2, 0, 0, 0, 0, 0, 8, 8, rows, None, ip), (fld, lab, 2, 0, 0, 0, 0, 8, 0, 8, rows, None, ip),
               (fld, lab, 2, 0, 0, 0, 0, 8, 8, 0, rows, None, ip),
               (fld, lab, 2, 0, 0, 0, 0, 9, 8, 8, rows, None, ip), (fld, lab, 2, 0, 0, 0, 0, 8, 9, 8, rows, None, ip),
               (fld, lab, 2, 0, 0, 0, 0, 8, 8, 9, rows, None, ip),                                   # larger than the container
               (fld, lab, 2, 0, 0, 0, 0, 32769, 1, 1, rows, None, ip), (fld, lab, 2, 0, 0, 0, 0, 32768, 32768, 2, rows, None, ip)]
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_label_field_sums" in hip.f3d_last_error()
        # n_labels * bins at the limit passes that check (and is then refused for its empty box: nothing that large is allocated); one
        # label more does not
        assert fn(fld, lab, 1 << 18, 0, 0, 1, 256, 0, 8, 8, rows, cp, ip) != 0 and b"empty box" in hip.f3d_last_error()
        assert fn(fld, lab, (1 << 18) + 1, 0, 0, 1, 256, 0, 8, 8, rows, cp, ip) != 0 and b"2^26" in hip.f3d_last_error()
        assert fn(fld, lab, 1 << 22, 0, 0, 1, 16, 0, 8, 8, rows, cp, ip) != 0 and b"empty box" in hip.f3d_last_error()
        assert fn(fld, lab, 1 << 22, 0, 0, 1, 17, 0, 8, 8, rows, cp, ip) != 0 and b"2^26" in hip.f3d_last_error()
        raw = np.frombuffer(rows, np.uint8)
        assert raw.min() == SENTINEL == raw.max() and info.used == 55 and (counts == 0x7F7F7F7F).all()   # a refused call writes nothing
        assert fn(fld, lab, 2, 1, 0, 0, 0, 8, 8, 8, rows, None, ip) == 0 and info.used == 512 and rows[0].n == 512 and rows[1].n == 0
        assert rows[0].iq == 3 * 512 and rows[0].iqq_lo == 9 * 512 and rows[0].iqq_hi == 0 and rows[1].min_key == 0xFFFFFFFF
        assert fn(fld, lab, 1, 1, 1.0, 2.0, 2, 7, 6, 5, rows, cp, ip) == 0 and rows[0].n == 210 and counts[:2].tolist() == [0, 210]
    finally:
        box.free()


# ---- f3d_paint_labels ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("dims", [(1, 1, 1), (65, 5, 33), (130, 9, 70)], ids=ids)
def test_paint_labels(f3d, cases, dims, in_place):
    arrays, s = cases[dims, ("outside", "noise")]
    n_labels = s["n_labels"]
    w, h, d = dims
    rng = np.random.default_rng(5)
    values = rng.uniform(-1, 1, n_labels).astype(F32)
    bits = values.view(np.uint32)
    bits[0], bits[n_labels // 2], bits[-1] = 0x7FC12345, 0xFFC00001, 0x7F800001       # NaN payloads, a signalling one among them
    fn = f3d._paint_entry()
    label_box = np.asarray(arrays["label_box"])
    dc, hc, wc = label_box.shape
    box = f3d.Containers(wc, hc, dc)
    try:
        pl = box.new(label_box.view(F32))
        po = pl if in_place else box.new(np.full(label_box.shape, 7.0, F32))
        box.set_current()
        f3d.check(fn(pl, n_labels, values.ctypes.data_as(f3d._fp), po, w, h, d), "f3d_paint_labels")
        got = box.download(po, (wc, hc, dc)).view(np.uint32)
        kept = box.download(pl, (wc, hc, dc)).view(np.int32)
    finally:
        box.free()
    want = ref.paint_labels(arrays["labels"], values)
    assert np.array_equal(got[:d, :h, :w], want)
    outside = np.ones(label_box.shape, bool)
    outside[:d, :h, :w] = False
    assert (got[outside] == (1 if in_place else np.float32(7.0).view(np.uint32))).all()   # padding untouched
    if not in_place:
        assert np.array_equal(kept, label_box)
    if w * h * d > 100:
        labels = np.asarray(arrays["labels"])
        assert (want[(labels < 1) | (labels > n_labels)] == ref.QUIET_NAN).all() and (want == 0x7FC12345).any()


def test_paint_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._paint_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        lab = box.new(np.ones((8, 8, 8), np.int32).view(F32))
        out = box.new(np.full((8, 8, 8), 7.0, F32))
        box.set_current()
        values = np.array([2.5, 3.5], F32)
        vp = values.ctypes.data_as(f3d._fp)
        for args in ((0, 2, vp, out, 8, 8, 8), (lab, 2, None, out, 8, 8, 8), (lab, 2, vp, 0, 8, 8, 8), (lab, 0, vp, out, 8, 8, 8),
                     (lab, (1 << 22) + 1, vp, out, 8, 8, 8), (lab, 2, vp, out, 0, 8, 8), (lab, 2, vp, out, 8, 8, 0), (lab, 2, vp, out, 9, 8, 8),
                     (lab, 2, vp, out, 8, 8, 9), (lab, 2, vp, out, 32769, 1, 1)):
            assert fn(*args) != 0, args
            assert b"f3d_paint_labels" in hip.f3d_last_error()
        assert (box.download(out, (8, 8, 8)) == 7.0).all()
        assert fn(lab, 2, vp, out, 8, 8, 8) == 0 and (box.download(out, (8, 8, 8)) == 2.5).all()
    finally:
        box.free()


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------------

def test_label_field_stats_from_anywhere(f3d, cases):
    dims, case = (65, 5, 33), ("outside", "noise")
    arrays, s = cases[dims, case]
    labels, field, n_labels = np.asarray(arrays["labels"]), np.asarray(arrays["field"]), s["n_labels"]
    sums = f3d.label_field_sums(field, labels, n_labels, shift=s["shift"], bins=64, range=(s["lo"], s["hi"]))
    check_rows(sums.rows, np.asarray(arrays["rows_64"]))
    assert np.array_equal(sums.counts, arrays["counts_64"]) and sums.info == s["info"]
    stats = f3d.solve_label_field(sums, min_voxels=5)
    want, summary = ref.solve(sums.rows, sums.counts, s["shift"], s["lo"], s["hi"], 64, 5)
    assert stats.rows.tobytes() == want.tobytes()
    assert {k: v for k, v in stats.summary.items() if k != "mean"} == {k: v for k, v in summary.items() if k != "mean"}
    assert stats.summary["mean"] == summary["mean"] and len(stats.as_table()) == n_labels
    # shift and range left open: the finite range under the labels, nothing finite out of range
    wide = f3d.label_field_stats(field, labels, n_labels, bins=32)          # 3e38 - (-3e38) overflows float32: no range for bins
    assert wide.bins == 0 and "not finite" in wide.info["note"] and wide.shift == -100
    field = np.where(np.isfinite(field) & (np.abs(field) > 1e30), F32(0), field)   # NaN and the infinities stay
    auto = f3d.label_field_stats(field, labels, n_labels, bins=32)
    lo, hi, found = ref.href.value_range(field, mask=labels)
    assert auto.shift == ref.shift_of(lo, hi, found["finite"]) and (auto.lo, auto.hi) == (float(lo), float(hi))
    rows, counts, info = ref.label_field_sums(field, labels, n_labels, auto.shift, lo, hi, 32)
    assert auto.info == info and np.array_equal(auto.counts, counts) and auto.n.tolist() == rows["n"].tolist()
    assert info["out_of_range"] >= int(np.isinf(field[(labels >= 1) & (labels <= n_labels)]).sum()) > 0
    flat = f3d.label_field_stats(np.full(field.shape, 2.0, F32), labels, n_labels, bins=32)
    assert flat.bins == 0 and flat.counts is None and "constant" in flat.info["note"] and (flat.mean[flat.n > 0] == 2.0).all()
    # the mean painted back
    painted = f3d.paint_labels(auto.mean, labels)
    body = (labels >= 1) & (labels <= n_labels)
    assert np.array_equal(painted[body].view(np.uint32), auto.mean.astype(F32)[labels[body] - 1].view(np.uint32))
    assert np.isnan(painted[~body]).all()


def test_the_driver_on_a_held_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        bodies = flow.segment(lo="otsu", min_voxels=8)
        assert bodies.n_labels > 3
        with pytest.raises(f3d.F3dError, match="eq"):                      # no strain yet
            flow.label_field("eq")
        grey = flow.label_field("grey", bins=16)                           # before any solve
        anywhere = f3d.label_field_stats(f0, bodies.labels, bodies.n_labels, bins=16)
        assert grey.rows.tobytes() == anywhere.rows.tobytes() and grey.info == anywhere.info and np.array_equal(grey.counts, anywhere.counts)
        assert grey.n.tolist() == bodies.sizes.tolist() and grey.summary == anywhere.summary
        flow.compute_resident(silent=True, warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)
        eq = flow.strain(fields=("eq",))["eq"]
        held = flow.label_field("eq", bins=64, min_voxels=20)
        anywhere = f3d.label_field_stats(eq, bodies.labels, bodies.n_labels, bins=64, min_voxels=20)
        assert held.rows.tobytes() == anywhere.rows.tobytes() and held.info == anywhere.info and np.array_equal(held.counts, anywhere.counts)
        assert held.shift == anywhere.shift and (held.lo, held.hi) == (anywhere.lo, anywhere.hi) and held.summary["ok"] > 0
        assert flow.label_field(eq, bins=64, min_voxels=20).rows.tobytes() == held.rows.tobytes()      # an array instead of a name
        painted = flow.paint_labels(held.mean)
        assert np.array_equal(painted.view(np.uint32), f3d.paint_labels(held.mean, bodies.labels).view(np.uint32))
        with pytest.raises(ValueError):
            flow.label_field("eq", bins=257)
        with pytest.raises(f3d.F3dError, match="nothing"):
            flow.label_field("nothing")
        flow.segment_end()
    finally:
        flow.destroy()


# ---- bin/flow3d --label-stats ---------------------------------------------------------------------------------------------------------------------

LINE = re.compile(r"label stats (\w+) frame 0(?: -> frame 1)?: (\d+) ok, (\d+) empty, (\d+) small of (\d+) labels, mean (\S+); shift (-?\d+), "
                  r"(\d+) bins over \[(\S+), (\S+)\]; (\d+) voxels used, (\d+) nan, (\d+) out of range, (\d+) foreign")
HEADER = "field,label,status,n,min,max,mean,std,q05,median,q95,below,above"


def test_cli_label_stats_of_a_pair(f3d, tmp_path):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([f0, f1]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", "4", "--outer", "2", "--inner", "3", "--silent", "--frames", *paths]

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    base = ["--segment", "otsu:", "--segment-min-voxels", "8", "--strain", "eq"]
    with_stats = run("s", base + ["--label-stats", "grey,eq", "--label-stats-paint"])
    plain = run("p", base)
    lines = {m[0]: m for m in LINE.findall(with_stats)}
    assert sorted(lines) == ["eq", "grey"] and not LINE.findall(plain)
    assert with_stats.index("bodies frame 0") < with_stats.index("label stats grey") < with_stats.index("strain frame 0")
    assert with_stats.index("strain frame 0") < with_stats.index("label stats eq")
    suffix = f"-{w}-{h}-{d}.raw"
    names = sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("p_"))
    new = ["labelstats.csv", "labelmean-grey" + suffix, "labelmean-eq" + suffix]
    assert sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("s_")) == sorted(names + new)
    assert "bodies.csv" in names and "labels.raw" in names and "strain-eq" + suffix in names
    for name in names:                                                     # every other output byte for byte
        assert open(tmp_path / f"s_{name}", "rb").read() == open(tmp_path / f"p_{name}", "rb").read(), name
    labels = np.fromfile(str(tmp_path / "s_labels.raw"), "<i4").reshape(d, h, w)
    n_labels = int(labels.max())
    assert n_labels > 3
    eq = np.fromfile(str(tmp_path / ("s_strain-eq" + suffix)), "<f4").reshape(d, h, w)
    rows = open(tmp_path / "s_labelstats.csv").read().strip().split("\n")
    assert rows[0] == HEADER and len(rows) == 1 + 2 * n_labels
    for k, (name, field) in enumerate((("grey", f0), ("eq", eq))):
        stats = f3d.label_field_stats(field, labels, n_labels, bins=64)
        for i, row in enumerate(rows[1 + k * n_labels:1 + (k + 1) * n_labels]):
            cells = row.split(",")
            assert len(cells) == 13 and cells[:3] == [name, str(i + 1), f3d.LABEL_STATUS[stats.status[i]]]
            assert [int(cells[3]), int(cells[11]), int(cells[12])] == [stats.n[i], stats.below[i], stats.above[i]]
            exp = [stats.min[i], stats.max[i], stats.mean[i], stats.std[i], stats.q05[i], stats.median[i], stats.q95[i]]
            assert np.allclose([float(c) for c in cells[4:11]], exp, rtol=1e-8, atol=0, equal_nan=True), (row, exp)
        line = lines[name]
        assert [int(line[j]) for j in (1, 2, 3, 4)] == [stats.summary["ok"], stats.summary["empty"], stats.summary["small"], n_labels]
        assert float(line[5]) == pytest.approx(stats.summary["mean"], rel=1e-8) and int(line[6]) == stats.shift and int(line[7]) == stats.bins == 64
        assert [int(line[j]) for j in (10, 11, 12, 13)] == [stats.info[c] for c in ("used", "nan", "out_of_range", "foreign")]
        painted = np.fromfile(str(tmp_path / f"s_labelmean-{name}{suffix}"), "<f4").reshape(d, h, w)
        values = np.where(stats.status == 0, stats.mean, np.nan).astype(F32)
        assert np.array_equal(painted.view(np.uint32), f3d.paint_labels(values, labels).view(np.uint32))
        assert np.isnan(painted[labels == 0]).all() and np.isfinite(painted[labels > 0]).all()
    # labels from a file, grey alone, no bins
    label_path = str(tmp_path / "labels.raw")
    labels.astype("<i4").tofile(label_path)
    out = run("a", ["--labels", label_path, "--label-stats", "grey", "--label-stats-bins", "0"])
    found = LINE.findall(out)
    assert len(found) == 1 and found[0][0] == "grey" and int(found[0][7]) == 0
    rows_a = open(tmp_path / "a_labelstats.csv").read().strip().split("\n")
    assert rows_a[0] == HEADER and len(rows_a) == 1 + n_labels and [r.split(",")[:8] for r in rows_a[1:]] == [r.split(",")[:8] for r in rows[1:1 + n_labels]]
    assert all(r.split(",")[8:11] == ["nan", "nan", "nan"] for r in rows_a[1:])
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("a_")) == sorted(["a_labelstats.csv"] + [f"a_flow-{c}{suffix}" for c in "uvw"])
