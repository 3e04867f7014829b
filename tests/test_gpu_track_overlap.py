"""The overlap of two label volumes through a displacement on the GPU: f3d_label_overlap against its numpy restatement
(tests/overlap_ref.py), never against itself, every field of every row and every counter bit for bit; the capacity rules; the
refusals; f3d_relabel_labels; the diagonal against f3d_label_shape_sums; track_labels; OpticalFlow.segment_next and .track on a held
flow and on a trajectory; and bin/flow3d --track in a three-frame sequence whose other outputs stay byte for byte the same.

Bounds.  Every word is an exact integer and the landing voxel is fixed by float32 operations the restatement repeats: equality,
whatever the schedule, and two calls give the same bytes.

Shapes.  The kernel's tile is 64 x 4 x 32 (a wave covers 64 x, a workgroup 4 rows, a run 32 planes): 64x4x32 is exactly one tile,
65x5x33 one voxel more along every axis; 130x9x70 has three tiles along every axis; 1x1x1, 2x2x2 and 3x70x2 are thinner than a tile.
The layout "seams" ends bodies exactly where the tiles end and changes the key on the last plane of a tile.  The LDS table has 128
slots: the 1000 x 1000 random labels give every run a key of its own, so runs close past it into the global table.

Padding.  The volume lies in the corner of containers three columns, two rows and a plane larger.  The padding of the label
containers carries a body's number and that of u, v, w NaN (the bytes between width and pitch are 0xFF): a kernel that reads padding
counts voxels that are not there.

Host memory and the module's name.  The name makes it sort behind tests/test_gpu_pipeline.py, whose page-locked test is sensitive to
what ran in the process before it (LABBOOK.md).  For the same reason the restatement runs in a child interpreter, once for all cases,
and the tests read its volumes, containers and rows as read-only file mappings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SENTINEL = 0x7F
SHAPES = [(1, 1, 1), (2, 2, 2), (64, 4, 32), (65, 5, 33), (3, 70, 2), (130, 9, 70)]
LAYOUTS = ("one", "same", "other", "random", "onekey", "mix", "seams")
EVERY = [(dims, layout, kind) for dims in SHAPES for layout in LAYOUTS for kind in ("none", "mixed")]
FIELDS = [(dims, "other", kind) for dims in ((65, 5, 33), (130, 9, 70)) for kind in ref.DISPLACEMENTS if kind not in ("none", "mixed")]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(dims, layout, kind) -> (arrays, info): every case computed once, by a child interpreter, and read as read-only file mappings
    (overlap_ref.in_child says why)"""
    keys = EVERY + FIELDS
    made = ref.in_child([[list(dims), layout, kind] for dims, layout, kind in keys], str(tmp_path_factory.mktemp("overlap_cases")))
    return dict(zip(keys, made))


def device_overlap(f3d, arrays, info, dims, capacity=None, calls=1):
    """f3d_label_overlap on the volume `dims` in the corner of the case's containers: (rows as a structured array over the whole room,
    info dict) per call; the room is filled with the sentinel byte before every call"""
    w, h, d = dims
    fn = f3d._overlap_entry()
    dc, hc, wc = arrays["container_a"].shape
    box = f3d.Containers(wc, hc, dc)
    try:
        pa, pb = box.new(arrays["container_a"].view(F32)), box.new(arrays["container_b"].view(F32))
        pd = [box.new(arrays["container_" + c]) for c in "uvw"] if "container_u" in arrays else [0, 0, 0]
        box.set_current()
        capacity = max(1, info["n_pairs"]) if capacity is None else capacity
        out = []
        for _ in range(calls):
            rows, counted = (f3d.Overlap * capacity)(), f3d.OverlapInfo()
            C.memset(rows, SENTINEL, C.sizeof(rows))
            f3d.check(fn(pa, info["n_a"], pb, info["n_b"], *pd, w, h, d, capacity, rows, C.byref(counted)), "f3d_label_overlap")
            out.append((np.frombuffer(rows, ref.ROWS_DTYPE), counted.as_dict()))          # a view, not a copy
    finally:
        box.free()
    return out if calls > 1 else out[0]


def check_rows(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() == np.asarray(want).tobytes():
        return
    for name in ref.ROWS_DTYPE.names:                                     # say which word of which row differs
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, (name, "row", int(bad[0][0]), got[bad[0][0]], want[bad[0][0]])


def untouched(rows):
    return rows.size == 0 or (np.frombuffer(rows.tobytes(), np.uint8) == SENTINEL).all()


def check_case(f3d, cases, key):
    dims = key[0]
    arrays, info = cases[key]
    want = arrays["rows"]
    counters = {k: v for k, v in info.items() if k not in ("n_a", "n_b")}
    (first, got), (second, got2) = device_overlap(f3d, arrays, info, dims, calls=2)
    assert first.tobytes() == second.tobytes() and got == got2            # two calls, identical bytes
    assert got == counters
    n = info["n_pairs"]
    check_rows(first[:n], want)
    assert untouched(first[n:])
    w, h, d = dims
    assert sum(got[c] for c in ref.CLASSES) == w * h * d and int(first["n"][:n].sum()) == got["lost_body"] + got["overlap"]
    return first[:n], got


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,layout,kind", EVERY, ids=ids)
def test_rows_equal_the_restatement_bit_for_bit(f3d, cases, dims, layout, kind):
    rows, info = check_case(f3d, cases, (dims, layout, kind))
    w, h, d = dims
    if kind == "none":
        assert info["lost_body"] == info["lost_background"] == 0 and (rows["ca2"] == rows["cb2"]).all()
        if layout in ("one", "onekey"):
            assert len(rows) == 1 and int(rows["n"][0]) == w * h * d and (rows["a"][0], rows["b"][0]) == ((1, 1) if layout == "one" else (3, 2))
        if layout == "same":
            assert (rows["a"] == rows["b"]).all()
    if w * h * d > 1000:
        assert (info["foreign_a"] > 0 and info["foreign_b"] > 0 and info["background"] > 0) == (layout == "mix")
        if kind == "mixed":
            assert info["lost_body"] > 0 and (rows["b"] == -1).any() and (rows["cb2"][rows["b"] == -1] == 0).all()
        if layout == "random":
            assert len(rows) > 0.9 * info["overlap"]                         # nearly every voxel a key of its own
        if layout == "mix":
            assert (rows["a"] == 0).any() and (rows["b"] == 0).any()


@pytest.mark.parametrize("dims,layout,kind", FIELDS, ids=ids)
def test_every_displacement(f3d, cases, dims, layout, kind):
    rows, info = check_case(f3d, cases, (dims, layout, kind))
    w, h, d = dims
    if kind == "zero":
        assert info["lost_body"] == 0 and (rows["ca2"] == rows["cb2"]).all()
    if kind == "shift":
        shift = (rows["cb2"] - rows["ca2"])[rows["b"] >= 0] / (2.0 * rows["n"][rows["b"] >= 0, None])
        assert (shift == [2, -1, 3]).all() and info["lost_body"] == w * h * d - (w - 2) * (h - 1) * (d - 3)
    if kind.startswith("out"):                                            # 3.25 voxels towards one face: four planes leave, and only they
        axis = "xyz".index(kind[4])
        assert info["lost_body"] == 4 * w * h * d // dims[axis] and len(set(rows["a"][rows["b"] == -1].tolist())) > 1
    if kind == "nan":
        assert info["lost_body"] > 0.1 * w * h * d


# ---- the capacity ----------------------------------------------------------------------------------------------------------------------------

def test_capacity_exact_one_short_and_far_too_small(f3d, cases):
    dims = (65, 5, 33)
    arrays, info = cases[dims, "other", "smooth"]
    n = info["n_pairs"]
    classes = {c: info[c] for c in ref.CLASSES}
    rows, got = device_overlap(f3d, arrays, info, dims, capacity=n)
    assert got["complete"] == 1 and got["n_pairs"] == n > 40 and got["table_lost"] == 0
    check_rows(rows, arrays["rows"])
    rows, got = device_overlap(f3d, arrays, info, dims, capacity=n - 1)       # the table itself has room: every key is counted
    assert got["complete"] == 0 and got["n_pairs"] == n and got["table_lost"] == 0 and untouched(rows)
    assert {c: got[c] for c in ref.CLASSES} == classes
    rows, got = device_overlap(f3d, arrays, info, dims, capacity=n + 7)
    assert got["complete"] == 1 and untouched(rows[n:])
    check_rows(rows[:n], arrays["rows"])
    arrays, info = cases[dims, "random", "mixed"]                              # two slots for thousands of keys
    rows, got = device_overlap(f3d, arrays, info, dims, capacity=1)
    assert got["complete"] == 0 and got["n_pairs"] <= 2 and untouched(rows)
    assert got["table_lost"] >= info["lost_body"] + info["overlap"] - 2 * int(arrays["rows"]["n"].max()) > 0   # at most two keys found a slot
    assert {c: got[c] for c in ref.CLASSES} == {c: info[c] for c in ref.CLASSES}


def test_the_binding_doubles_the_capacity(f3d, cases):
    dims = (130, 9, 70)
    arrays, info = cases[dims, "random", "none"]
    assert info["n_pairs"] > 4 * 8 * 2000                                      # the first capacity, 8 * (n_a + n_b), is far too small
    found = f3d.label_overlap(arrays["labels_a"], arrays["labels_b"], n_a=info["n_a"], n_b=info["n_b"])
    assert found.info == {k: v for k, v in info.items() if k not in ("n_a", "n_b")} and len(found) == info["n_pairs"]
    want = arrays["rows"]
    assert found.a.tolist() == want["a"].tolist() and found.b.tolist() == want["b"].tolist() and (found.n == want["n"]).all()
    assert (found.ca2 == want["ca2"]).all() and (found.cb2 == want["cb2"]).all()
    short = f3d.label_overlap(arrays["labels_a"], arrays["labels_b"], n_a=info["n_a"], n_b=info["n_b"], capacity=100)
    assert len(short) == 0 and short.info["complete"] == 0 and short.info["overlap"] == info["overlap"]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._overlap_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        la, lb = (box.new(np.ones((8, 8, 8), np.int32).view(F32)) for _ in range(2))
        u, v, w = (box.new(np.zeros((8, 8, 8), F32)) for _ in range(3))
        box.set_current()
        rows, info = (f3d.Overlap * 4)(), f3d.OverlapInfo()
        C.memset(rows, SENTINEL, C.sizeof(rows))
        info.overlap = 55
        size, tail = (8, 8, 8), (4, rows, C.byref(info))
        big = (1 << 22) + 1
        bad = [(0, 1, lb, 1, 0, 0, 0, *size, *tail), (la, 1, 0, 1, 0, 0, 0, *size, *tail), (la, 1, lb, 1, 0, 0, 0, *size, 4, None, C.byref(info)),
               (la, 1, lb, 1, 0, 0, 0, *size, 4, rows, None),
               (la, 1, lb, 1, u, 0, 0, *size, *tail), (la, 1, lb, 1, u, v, 0, *size, *tail), (la, 1, lb, 1, 0, v, w, *size, *tail),
               (la, 0, lb, 1, 0, 0, 0, *size, *tail), (la, big, lb, 1, 0, 0, 0, *size, *tail), (la, 1, lb, 0, 0, 0, 0, *size, *tail),
               (la, 1, lb, big, 0, 0, 0, *size, *tail),
               (la, 1, lb, 1, 0, 0, 0, *size, 0, rows, C.byref(info)), (la, 1, lb, 1, 0, 0, 0, *size, (1 << 24) + 1, rows, C.byref(info)),
               (la, 1, lb, 1, 0, 0, 0, 0, 8, 8, *tail), (la, 1, lb, 1, 0, 0, 0, 8, 0, 8, *tail), (la, 1, lb, 1, 0, 0, 0, 8, 8, 0, *tail),
               (la, 1, lb, 1, 0, 0, 0, 9, 8, 8, *tail), (la, 1, lb, 1, 0, 0, 0, 8, 9, 8, *tail), (la, 1, lb, 1, 0, 0, 0, 8, 8, 9, *tail),
               (la, 1, lb, 1, 0, 0, 0, 32769, 1, 1, *tail), (la, 1, lb, 1, 0, 0, 0, 1, 1, 32769, *tail),
               (la, 1, lb, 1, 0, 0, 0, 32768, 32768, 16, *tail),
               (la, 1, la, 1, 0, 0, 0, *size, *tail),                                                   # one container for both
               (la, 1, lb, 1, la, v, w, *size, *tail), (la, 1, lb, 1, u, lb, w, *size, *tail), (la, 1, lb, 1, u, v, lb, *size, *tail)]
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_label_overlap" in hip.f3d_last_error(), hip.f3d_last_error()
        assert b"container of labels_b" in hip.f3d_last_error()
        raw = np.frombuffer(rows, np.uint8)
        assert raw.min() == SENTINEL == raw.max() and info.overlap == 55     # a refused call writes nothing
        assert fn(la, 1, lb, 1, u, v, w, *size, *tail) == 0 and info.overlap == 512 and info.n_pairs == 1 and info.complete == 1
        assert (rows[0].a, rows[0].b, rows[0].n, list(rows[0].ca2), list(rows[0].cb2)) == (1, 1, 512, [0, 0, 0], [0, 0, 0])
        assert fn(la, 1, lb, 1, 0, 0, 0, 7, 6, 5, *tail) == 0 and rows[0].n == 210                    # a volume smaller than the container
        relabel = f3d._relabel_entry()
        m = (C.c_int * 2)(1, 2)
        minus = (C.c_int * 2)(1, -1)
        count = C.c_ulonglong(77)
        for args in ((0, 2, m, lb, *size, C.byref(count)), (la, 2, None, lb, *size, C.byref(count)), (la, 2, m, 0, *size, C.byref(count)),
                     (la, 0, m, lb, *size, C.byref(count)), (la, big, m, lb, *size, C.byref(count)), (la, 2, minus, lb, *size, C.byref(count)),
                     (la, 2, m, lb, 9, 8, 8, C.byref(count)), (la, 2, m, lb, 8, 8, 0, C.byref(count))):
            assert relabel(*args) != 0, args
            assert b"f3d_relabel_labels" in hip.f3d_last_error()
        assert count.value == 77 and (box.download(lb, size).view(np.int32) == 1).all()
    finally:
        box.free()


# ---- f3d_relabel_labels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (65, 5, 33), (130, 9, 70)], ids=ids)
def test_relabel_against_the_restatement(f3d, cases, dims):
    arrays, info = cases[dims, "mix", "none"]
    w, h, d = dims
    n = info["n_a"]
    rng = np.random.default_rng(5)
    mapping = rng.integers(0, 90, n).astype(np.int32)
    mapping[:4] = [7, 7, 0, 2 ** 31 - 1]                                       # two labels merge, one goes to the background
    want, foreign = ref.relabel(arrays["labels_a"], mapping)
    fn = f3d._relabel_entry()
    container = arrays["container_a"]
    dc, hc, wc = container.shape
    box = f3d.Containers(wc, hc, dc)
    try:
        src, dst = box.new(container.view(F32)), box.new(np.full(container.shape, -5, np.int32).view(F32))
        box.set_current()
        count = C.c_ulonglong()
        f3d.check(fn(src, n, mapping.ctypes.data_as(C.POINTER(C.c_int)), dst, w, h, d, C.byref(count)), "f3d_relabel_labels")
        out = box.download(dst, (wc, hc, dc)).view(np.int32)
        assert count.value == foreign and (out[:d, :h, :w] == want).all()
        out[:d, :h, :w] = -5
        assert (out == -5).all()                                              # padding is not written
        f3d.check(fn(src, n, mapping.ctypes.data_as(C.POINTER(C.c_int)), src, w, h, d, None), "f3d_relabel_labels")   # in place
        back = box.download(src, (wc, hc, dc)).view(np.int32)
        assert (back[:d, :h, :w] == want).all()
        back[:d, :h, :w] = n
        assert (back == n).all()
    finally:
        box.free()
    got, counted = f3d.relabel_labels(arrays["labels_a"], mapping, count_foreign=True)
    assert got.dtype == np.int32 and (got == want).all() and counted == foreign and (foreign > 0 or w * h * d < 1000)


def test_the_diagonal_is_the_voxel_count_of_label_shape_sums(f3d, cases):
    dims = (65, 5, 33)
    arrays, info = cases[dims, "same", "none"]
    found = f3d.label_overlap(arrays["labels_a"], arrays["labels_b"], n_a=info["n_a"], n_b=info["n_b"])
    sums, shape_info = f3d.label_shape_sums(arrays["labels_a"], info["n_a"])
    present = np.nonzero(sums["n"])[0] + 1
    assert found.a.tolist() == found.b.tolist() == present.tolist() and found.n.tolist() == sums["n"][present - 1].tolist()
    assert found.info["overlap"] == shape_info["labelled"] and found.matrix()[(int(present[0]), int(present[0]))] == int(found.n[0])
    dense = found.matrix(info["n_a"], info["n_b"])
    assert dense.shape == (41, 42) and dense.sum() == shape_info["labelled"] and (np.diag(dense[1:, 2:]) == sums["n"]).all()
    N = [k - 1 for k in dims]                                                  # the doubled moments: 2 s1 - (N - 1) n
    assert (found.ca2 == 2 * sums["s1"][present - 1].astype(np.int64) - np.outer(sums["n"][present - 1].astype(np.int64), N)).all()


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------------

def test_track_labels_on_blocks_one_of_which_breaks(f3d):
    a = np.zeros((12, 20, 40), np.int32)
    b = np.zeros_like(a)
    a[2:8, 2:8, 2:14], a[2:8, 11:17, 2:10] = 1, 2
    b[2:8, 2:8, 5:11], b[2:8, 2:8, 12:17] = 2, 1                              # body 1 moved by 3 and broke; the pieces are 6 and 5 wide
    b[2:8, 11:17, 1:9] = 3                                                     # body 2 moved by -1
    b[9:11, 2:4, 30:33] = 4                                                    # and something new
    u = np.where(a == 1, 3, np.where(a == 2, -1, 0)).astype(F32)
    zero = np.zeros(a.shape, F32)
    tracks = f3d.track_labels(a, b, u, zero, zero, min_fraction=0.2)
    want_rows, want_info = ref.label_overlap(a, 2, b, 4, u, zero, zero)
    want_a, want_b, want_map, want_summary = ref.solve(want_rows, 2, 4, 0.2)
    assert tracks.info == want_info and tracks.a.tobytes() == want_a.tobytes() and tracks.b.tobytes() == want_b.tobytes()
    assert tracks.map_b.tolist() == want_map.tolist() == [3, 1, 2, 4] and tracks.summary == want_summary
    assert tracks.summary == dict(matched=2, split=1, merged=0, vanished=0, appeared=1, left=0, n_ids=4)
    # body 2 lands on x 1 .. 8 of B's body 3, whose column x = 1 is also reached by the background voxels that stayed: m = 288 + 36
    assert tracks.a["shift"].tolist() == [[3, 0, 0], [-1, 0, 0]] and tracks.a["iou"][1] == 288 / 324 and tracks.b["n_unreached"][2] == 36
    assert (tracks.relabelled == ref.relabel(b, want_map)[0]).all() and (tracks.relabelled[b == 2] == 1).all()
    assert [r["status"] for r in tracks.as_table()[:2]] == [["matched", "split"], ["matched"]]


def solve_pair(f3d, flow, frames):
    flow.upload(*frames)
    flow.compute_resident(silent=True, warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)


@pytest.mark.parametrize("source", ["flow", "trajectory"])
def test_segment_next_and_track_on_the_driver(f3d, source):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        with pytest.raises(ValueError, match="there was none"):
            flow.segment_next()
        if source == "trajectory":
            flow.trajectory_begin()
        solve_pair(f3d, flow, (f0, f1))
        if source == "trajectory":
            flow.trajectory_append()
            disp = flow.trajectory_download()[:3]
        else:
            disp = flow.download()
        with pytest.raises(f3d.F3dError, match="label"):                      # neither volume is on the device yet
            flow.track(n_a=3, n_b=3)
        bodies = flow.segment(lo="otsu", min_voxels=8)
        with pytest.raises(f3d.F3dError, match="second label volume"):
            flow.track(n_b=3)
        later = flow.segment_next()                                            # the cut of frame 0, as a number, on frame 1
        lo, hi, min_voxels, _ = flow._segment_settled
        anywhere = f3d.label_components(f1, lo, hi, min_voxels)
        assert (later.labels == anywhere.labels).all() and later.sizes.tolist() == anywhere.sizes.tolist() and later.info == anywhere.info
        assert later.n_labels > 3 and bodies.n_labels > 3
        tracks = flow.track(source=source)
        want = f3d.track_labels(bodies.labels, later.labels, *disp, n_a=bodies.n_labels, n_b=later.n_labels)
        assert tracks.info == want.info and tracks.a.tobytes() == want.a.tobytes() and tracks.b.tobytes() == want.b.tobytes()
        assert tracks.map_b.tolist() == want.map_b.tolist() and tracks.summary == want.summary
        assert (tracks.relabelled == want.relabelled).all() and tracks.summary["matched"] > 0
        rows, info = ref.label_overlap(bodies.labels, bodies.n_labels, later.labels, later.n_labels, *disp)
        assert tracks.info == info and tracks.overlaps.n.tolist() == rows["n"].tolist() and tracks.overlaps.a.tolist() == rows["a"].tolist()
        assert (tracks.overlaps.cb2 == rows["cb2"]).all()
        # labels of the later frame from the caller, no renumbering; then a split on the later frame
        given = flow.track(later.labels, source=source, n_a=bodies.n_labels, relabel=False)
        assert given.relabelled is None and given.a.tobytes() == tracks.a.tobytes()
        split = flow.segment_next(lo, hi, min_voxels, split=2)
        assert "n_cores" in split.info and (split.labels == f3d.split_components(f1, lo, hi, core_d2=2, min_voxels=min_voxels).labels).all()
        with pytest.raises(ValueError, match="numbers"):
            flow.segment_next(lo="otsu")
        with pytest.raises(ValueError):
            flow.track(later.labels[:, :, :-1])
        flow.track_end()
        flow.segment_end()
    finally:
        flow.destroy()


# ---- bin/flow3d --track -----------------------------------------------------------------------------------------------------------------------

LINE = re.compile(r"track frame (\d+) -> frame (\d+): (\d+) of (\d+) bodies matched, (\d+) split, (\d+) merged, (\d+) vanished, (\d+) appeared, "
                  r"(\d+) left; mean IoU (\S+); lost (\d+), foreign (\d+)")
HEADER = "side,label,status,voxels,lost,background,unreached,best,n_best,partners,fraction,shift_x,shift_y,shift_z,iou,new_label"


def test_cli_track_in_a_cumulative_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    frames = [s0, s1, s0]
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    cut = F32(f3d.histogram(s0).otsu(2).values[0])                         # the cut as a number: what --track repeats on every frame
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", "4", "--outer", "2", "--inner", "3", "--silent", "--frames", *paths,
            "--cumulative", "--segment", "%.9g:" % cut, "--segment-min-voxels", "8", "--contacts"]

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    tracked = run("t", ["--track", "--track-min-fraction", "0.25"])
    plain = run("p", [])
    lines = LINE.findall(tracked)
    assert len(lines) == 2 and not LINE.findall(plain) and [l[:2] for l in lines] == [("0", "1"), ("0", "2")]
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("bodies frame", "displacement frame", "contacts frame"))]
    assert keep(tracked) == keep(plain) and len(keep(plain)) >= 4
    names = sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("p_"))
    extra = [f"{k}_{what}" for k in (0, 1) for what in ("tracks.csv", "tracked-labels.raw")]
    assert sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("t_")) == sorted(names + extra)
    assert "0_labels.raw" in names and len(names) >= 12
    for name in names:                                                     # every other output byte for byte
        assert open(tmp_path / f"t_{name}", "rb").read() == open(tmp_path / f"p_{name}", "rb").read(), name
    labels = np.fromfile(str(tmp_path / "t_0_labels.raw"), "<i4").reshape(d, h, w)
    n_a = int(labels.max())
    assert n_a > 3
    for k in (0, 1):
        later = f3d.label_components(frames[k + 1], float(cut), np.inf, 8)
        disp = [np.fromfile(str(tmp_path / f"t_{k}_disp-{c}-{w}-{h}-{d}.raw"), "<f4").reshape(d, h, w) for c in "uvw"]
        want = f3d.track_labels(labels, later.labels, *disp, min_fraction=0.25, n_a=n_a, n_b=later.n_labels)
        got = np.fromfile(str(tmp_path / f"t_{k}_tracked-labels.raw"), "<i4").reshape(d, h, w)
        assert (got == want.relabelled).all()
        table = open(tmp_path / f"t_{k}_tracks.csv").read().strip().split("\n")
        assert table[0] == HEADER and len(table) == 1 + n_a + later.n_labels
        for i, row in enumerate(table[1:1 + n_a]):
            cells = row.split(",")
            t = want.a[i]
            assert cells[:3] == ["a", str(i + 1), str(t["status"])] and int(cells[-1]) == i + 1
            assert [int(c) for c in cells[3:10]] == [t["n"], t["n_lost"], t["n_background"], 0, t["best_b"], t["n_best"], t["n_targets"]]
            assert np.allclose([float(c) for c in cells[10:15]], [t["fraction"], *t["shift"], t["iou"]], rtol=1e-8, equal_nan=True)
        for i, row in enumerate(table[1 + n_a:]):
            cells = row.split(",")
            t = want.b[i]
            assert cells[:3] == ["b", str(i + 1), str(t["status"])] and int(cells[-1]) == want.map_b[i]
            assert [int(c) for c in cells[3:10]] == [t["m"], 0, 0, t["n_unreached"], t["best_a"], t["n_best"], t["n_sources"]]
        s = want.summary
        assert [int(x) for x in lines[k][2:9]] == [s["matched"], n_a, s["split"], s["merged"], s["vanished"], s["appeared"], s["left"]]
        matched = (want.a["status"] & ref.MATCHED) != 0
        assert float(lines[k][9]) == pytest.approx(want.a["iou"][matched].mean(), rel=1e-5) and s["matched"] > 0
        assert [int(x) for x in lines[k][10:]] == [want.info["lost_body"] + want.info["lost_background"],
                                                   want.info["foreign_a"] + want.info["foreign_b"]]
