"""The connected bodies of a thresholded volume on the GPU: f3d_label_components against its numpy restatement (tests/components_ref.py),
never against itself, in containers three columns, two rows and a plane larger than the box.  The float padding of src is filled with a
FOREGROUND value (a read past the box would join bodies or change the counts) and labels_out with a sentinel that must survive
outside the box; the sizes array carries a sentinel behind what is handed out.

Bounds.  Everything is an integer that is a function of the input alone: labels_out, sizes and every counter of the info equal the
restatement bit for bit, and two calls give the same bytes.

Shapes: the kernels keep f3d_label_motion_sums' tile (a wave covers 64 x, a workgroup 4 rows, a lane 32 planes), so 65 x 5 x 33 is one
voxel past a tile along every axis and 130 x 9 x 70 has three tiles in x and z; 2x1x1, 1x2x1 and 1x1x2 have one face, each axis alone.
The seam volumes put two slabs exactly on either side of a tile boundary (x = 63|64 and 127|128, y = 3|4 and 7|8, z = 31|32 and 63|64).
The large case: the prefix sum works on block sums of kScanBlock * kScanItems = 1024 voxels and scans them kScanThreads = 1024 per trip
of its loop (csrc/f3d_label_components.hip; the test reads the three constants from there), so 160 x 96 x 72 = 1 105 920 voxels make
1080 block sums and two trips; its layouts have closed-form answers and no restatement runs at that size."""
import ctypes as C
import functools
import mmap
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SENTINEL = 0x7F
LABEL_SENTINEL = 0x7F7F7F7F
SIZE_SENTINEL = 0x7F7F7F7F7F7F7F7F
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (3, 2, 2), (65, 5, 33), (130, 9, 70)]        # (w, h, d)
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
INF = float("inf")


def poison_byte(lo, hi):
    """a byte whose four-fold repetition is a float inside [lo, hi]: the padding of src is foreground.  (Where no such byte exists --
    a range of denormals only, or of one infinity -- the padding is 0x3F3F3F3F and merely not NaN.)"""
    for b in [0x3F] + list(range(256)):
        v = np.frombuffer(bytes([b] * 4), F32)[0]
        if F32(lo) <= v <= F32(hi):
            return b
    return 0x3F


def device_components(f3d, volume, lo, hi, min_voxels, capacity=None, calls=1, keep_sizes=True):
    """f3d_label_components on a box in the corner of larger containers: per call (labels, sizes array with its tail, info dict, the
    whole label container).  capacity None: room for every voxel; keep_sizes False: a null sizes"""
    d, h, w = volume.shape
    fn = f3d._components_entry()
    box = f3d.Containers(w + 3, h + 2, d + 1)
    room = volume.size if capacity is None else capacity
    try:
        src = box.alloc(fill=poison_byte(lo, hi))
        box.upload(src, volume)
        box.set_current()
        out = []
        for _ in range(calls):
            dst = box.alloc(fill=SENTINEL)
            sizes = np.full(room + 3, SIZE_SENTINEL, np.uint64)
            info = f3d.ComponentInfo()
            ptr = sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)) if keep_sizes else None
            f3d.check(fn(src, lo, hi, min_voxels, dst, w, h, d, ptr, room if keep_sizes else 0, C.byref(info)), "f3d_label_components")
            whole = box.download(dst, (w + 3, h + 2, d + 1)).view(np.int32)
            out.append((whole[:d, :h, :w].copy(), sizes, info.as_dict(), whole))
    finally:
        box.free()
    return out if calls > 1 else out[0]


def check_call(got, want, shape):
    labels, sizes, info, whole = got
    want_labels, want_sizes, want_info = want
    d, h, w = shape
    assert info == want_info, (info, want_info)
    assert labels.dtype == np.int32 and np.array_equal(labels, want_labels)
    outside = np.ones(whole.shape, bool)
    outside[:d, :h, :w] = False
    assert (whole[outside] == LABEL_SENTINEL).all()                      # nothing written past the box
    n = len(want_sizes)
    assert np.array_equal(sizes[:n], want_sizes) and (sizes[n:] == SIZE_SENTINEL).all()
    assert info["foreground"] + info["background"] == d * h * w and info["n_components"] == info["n_labels"] + info["dropped_components"]


@functools.lru_cache(maxsize=None)
def base_case(dims, layout):
    """(volume, the restatement for min_voxels = 1): computed once, shared and left unchanged"""
    w, h, d = dims
    mask = ref.layout_mask(layout, (d, h, w))
    volume = ref.as_volume(mask, 0.75, 0.25)
    volume.setflags(write=False)
    return volume, ref.label_components(volume, 0.5, 1.0, 1)


# ---- the table -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_labels_sizes_and_info_equal_the_restatement_bit_for_bit(f3d, dims, layout):
    volume, base = base_case(dims, layout)
    largest = base[2]["largest"]
    for min_voxels in (1, 2, 27, largest + 1):
        want = ref.apply_min_voxels(*base, min_voxels)
        first, second = device_components(f3d, volume, 0.5, 1.0, min_voxels, calls=2)
        check_call(first, want, volume.shape)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]
        if min_voxels == largest + 1:
            assert want[2]["n_labels"] == 0 and not first[0].any()     # above the largest body: every label is 0
    w, h, d = dims
    if dims == SHAPES[-1]:
        assert (base[2]["n_labels"] == (w * h * d + 1) // 2) == (layout == "checker")          # every rank of the prefix sum
        assert (base[2]["n_labels"] == 1) == (layout in ("full", "serpentine", "serpentine-mirrored"))


@pytest.mark.parametrize("apart", [False, True], ids=["touching", "apart"])
@pytest.mark.parametrize("at", [1, 2], ids=["first-seam", "second-seam"])
@pytest.mark.parametrize("axis", [2, 1, 0], ids=["x", "y", "z"])
def test_two_slabs_at_the_seam_between_two_tiles(f3d, axis, at, apart):
    """a slab two voxels thick that ends with the last voxel of a tile and a slab one voxel thick that is the first plane of the next:
    one body when they meet across the seam, two when the first slab lies one voxel back and the last voxel of the tile is background"""
    w, h, d = 130, 9, 70
    seam = at * {2: 64, 1: 4, 0: 32}[axis]
    mask = np.zeros((d, h, w), bool)
    index = [slice(None)] * 3
    index[axis] = slice(seam - 3, seam - 1) if apart else slice(seam - 2, seam)
    mask[tuple(index)] = True
    index[axis] = seam
    mask[tuple(index)] = True
    volume = ref.as_volume(mask, 0.75, 0.25)
    want = ref.label_components(volume, 0.5, 1.0, 1)
    face = w * h * d // (w, h, d)[2 - axis]
    assert want[1].tolist() == ([2 * face, face] if apart else [3 * face])
    check_call(device_components(f3d, volume, 0.5, 1.0, 1), want, volume.shape)


# ---- values --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def special_volume():
    w, h, d = 65, 5, 33
    rng = np.random.default_rng(4)
    v = rng.random((d, h, w)).astype(F32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.25, 0.75, 0.0, -0.0, 1e-45, -1e-45, 1e-40, 0.5], F32)
    m = rng.random(v.shape) < 0.3
    v[m] = rng.choice(specials, size=int(m.sum()))
    v[10:14, 1:4, 20:40] = np.nan                                       # a NaN block, beside the NaN holes above
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("lo,hi", [(-INF, INF), (0.25, 0.75), (0.0, 0.5), (0.0, 0.0), (1e-45, 1e-40), (-INF, 0.3), (0.6, INF), (INF, INF),
                                   (-INF, -INF), (-1e-45, 1e-45)], ids=str)
def test_special_values_and_bounds(f3d, lo, hi):
    """NaN holes and a NaN block, +-inf with open and with finite bounds, values exactly lo and exactly hi, -0.0 with lo = 0, denormals"""
    v = special_volume()
    want = ref.label_components(v, lo, hi, 1)
    assert want[2]["nan"] == np.isnan(v).sum() > 80
    if (lo, hi) == (-INF, INF):
        assert want[2]["background"] == want[2]["nan"]
    if (lo, hi) == (0.0, 0.0):
        assert want[2]["foreground"] == (v == 0).sum() > 100 and np.signbit(v[v == 0]).any()     # 0.0 and -0.0 alike
    if (lo, hi) == (0.25, 0.75):
        assert (v[ref.foreground(v, lo, hi)] == F32(0.25)).any() and (v[ref.foreground(v, lo, hi)] == F32(0.75)).any()
    check_call(device_components(f3d, v, lo, hi, 1), want, v.shape)


# ---- min_voxels and sizes ------------------------------------------------------------------------------------------------------------

def test_min_voxels_exactly_a_size_and_one_above(f3d):
    volume, base = base_case((65, 5, 33), "noise-0.31")
    sizes = base[1]
    size = int(np.sort(np.unique(sizes))[len(np.unique(sizes)) // 2])    # a size in the middle that bodies do have
    assert (sizes == size).any() and 2 < size < base[2]["largest"]
    at, above = ref.apply_min_voxels(*base, size), ref.apply_min_voxels(*base, size + 1)
    assert at[2]["n_labels"] - above[2]["n_labels"] == (sizes == size).sum() > 0
    check_call(device_components(f3d, volume, 0.5, 1.0, size), at, volume.shape)
    check_call(device_components(f3d, volume, 0.5, 1.0, size + 1), above, volume.shape)
    check_call(device_components(f3d, volume, 0.5, 1.0, 2 ** 63), ref.apply_min_voxels(*base, 2 ** 63), volume.shape)


def test_the_capacity_of_sizes(f3d):
    volume, base = base_case((65, 5, 33), "voronoi")
    want = ref.apply_min_voxels(*base, 2)
    n = want[2]["n_labels"]
    assert n > 10
    for capacity in (n, n - 4, 1, n + 5):
        labels, sizes, info, whole = device_components(f3d, volume, 0.5, 1.0, 2, capacity=capacity)
        k = min(n, capacity)
        assert info == want[2] and np.array_equal(labels, want[0])
        assert np.array_equal(sizes[:k], want[1][:k]) and (sizes[k:] == SIZE_SENTINEL).all()     # the tail keeps its fill
    labels, sizes, info, whole = device_components(f3d, volume, 0.5, 1.0, 2, keep_sizes=False)   # a null sizes
    assert info == want[2] and np.array_equal(labels, want[0]) and (sizes == SIZE_SENTINEL).all()


def test_a_call_on_the_complement_carries_nothing_over(f3d):
    """the scratch buffer is reused: the complement of the mask directly afterwards, in the same containers, is right too"""
    volume, base = base_case((130, 9, 70), "noise-0.6")
    d, h, w = volume.shape
    fn = f3d._components_entry()
    box = f3d.Containers(w + 3, h + 2, d + 1)
    try:
        src = box.alloc(fill=0x3F)
        box.upload(src, volume)
        dst = box.alloc(fill=SENTINEL)
        box.set_current()
        info = f3d.ComponentInfo()
        got = []
        for lo, hi in ((0.5, 1.0), (0.0, 0.5), (0.5, 1.0)):
            f3d.check(fn(src, lo, hi, 1, dst, w, h, d, None, 0, C.byref(info)), "f3d_label_components")
            got.append((box.download(dst, (w, h, d)).view(np.int32), info.as_dict()))
    finally:
        box.free()
    complement = ref.label_components(volume, 0.0, 0.5, 1)
    assert np.array_equal(got[0][0], base[0]) and got[0][1] == base[2]
    assert np.array_equal(got[1][0], complement[0]) and got[1][1] == complement[2]
    assert np.array_equal(got[2][0], base[0]) and got[2][1] == base[2]


# ---- more than one trip of the scan of the block sums ------------------------------------------------------------------------------------

def scan_constants():
    text = open(os.path.join(ROOT, "cuda-flow3d_amd", "csrc", "f3d_label_components.hip")).read()
    return [int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("kScanBlock", "kScanItems", "kScanThreads")]


def large_slab(layout, dims, z0, z1, before):
    """planes z0 .. z1 of the large case in closed form: (mask, labels int32), `before` the labels handed out below z0 (checker)"""
    w, h, d = dims
    z, y, x = (np.arange(z0, z1, dtype=np.int32)[:, None, None], np.arange(h, dtype=np.int32)[None, :, None],
               np.arange(w, dtype=np.int32)[None, None, :])
    if layout == "checker":                                              # every foreground voxel a body: its label is the running count
        mask = (x + y + z) % 2 == 0
        labels = np.cumsum(mask.ravel(), dtype=np.int32).reshape(mask.shape) + np.int32(before)
    elif layout == "full":
        mask = np.ones((z1 - z0, h, w), bool)
        labels = np.ones(mask.shape, np.int32)
    else:                                                                # bricks of 7 x 5 x 3 voxels between one-voxel walls (ref.bricks)
        mask = (x % 8 != 7) & (y % 6 != 5) & (z % 4 != 3)
        labels = 1 + x // 8 + (w // 8) * (y // 6 + (h // 6) * (z // 4))
    return mask, np.where(mask, labels, 0).astype(np.int32)


@pytest.mark.parametrize("layout", ["checker", "full", "bricks"])
def test_the_scan_of_the_block_sums_takes_more_than_one_trip(f3d, layout):
    """kScanBlock * kScanItems voxels per block sum, kScanThreads block sums per trip: the shape has more block sums than one trip takes.
    Closed forms only: the running count of the mask (checker), one body (full), bricks of 7 x 5 x 3 between one-voxel walls.
    The volume goes up and the labels come down eight planes at a time and the sizes live in a mapping of their own: no host block of
    this test is larger than those of the small shapes (freed large blocks change where later tests' arrays live, LABBOOK.md)."""
    block, items, per_trip = scan_constants()
    w, h, d = dims = 160, 96, 72
    assert block * items * per_trip < w * h * d <= 2 ** 22 and w % 8 == 0 and h % 6 == 0 and d % 4 == 0
    step = 8
    n_labels = {"checker": w * h * d // 2, "full": 1, "bricks": (w // 8) * (h // 6) * (d // 4)}[layout]
    size = {"checker": 1, "full": w * h * d, "bricks": 7 * 5 * 3}[layout]
    foreground = n_labels * size
    fn = f3d._components_entry()
    box = f3d.Containers(w + 3, h + 2, d + 1)
    sizes = np.frombuffer(mmap.mmap(-1, (n_labels + 3) * 8), np.uint64)
    sizes[:] = SIZE_SENTINEL
    try:
        src = box.alloc(fill=0x3F)
        dst = box.alloc(fill=SENTINEL)
        before = 0
        for z0 in range(0, d, step):
            mask, _ = large_slab(layout, dims, z0, z0 + step, before)
            before += int(mask.sum())
            box.upload(src, ref.as_volume(mask, 0.75, 0.25), z0)
        assert before == foreground
        box.set_current()
        info = f3d.ComponentInfo()
        f3d.check(fn(src, 0.5, 1.0, 1, dst, w, h, d, sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)), n_labels, C.byref(info)),
                  "f3d_label_components")
        assert info.as_dict() == dict(foreground=foreground, background=w * h * d - foreground, nan=0, n_components=n_labels,
                                      n_labels=n_labels, dropped_components=0, dropped_voxels=0, largest=size)
        before = 0
        for z0 in range(0, d + 1, step):
            z1 = min(z0 + step, d + 1)
            got = box.download(dst, (w + 3, h + 2, z1 - z0), z0).view(np.int32)
            want = np.full(got.shape, LABEL_SENTINEL, np.int32)              # outside the box the fill survives
            if z0 < d:
                mask, want[:, :h, :w] = large_slab(layout, dims, z0, z1, before)
                before += int(mask.sum())
            assert np.array_equal(got, want), f"planes {z0} .. {z1}"
        assert (sizes[:n_labels] == size).all() and (sizes[n_labels:] == SIZE_SENTINEL).all()
    finally:
        box.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._components_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        src = box.new(np.full((8, 8, 8), 0.75, F32))
        dst = box.alloc(fill=SENTINEL)
        box.set_current()
        sizes = np.full(4, SIZE_SENTINEL, np.uint64)
        ps = sizes.ctypes.data_as(C.POINTER(C.c_ulonglong))
        info = f3d.ComponentInfo()
        info.largest = 55
        pi = C.byref(info)
        nan = float("nan")
        bad = [(0, 0.5, 1.0, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 1, 0, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 8, 8, 8, ps, 4, None),
               (src, 0.5, 1.0, 1, src, 8, 8, 8, ps, 4, pi),
               (src, nan, 1.0, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, nan, 1, dst, 8, 8, 8, ps, 4, pi), (src, 1.0, 0.5, 1, dst, 8, 8, 8, ps, 4, pi),
               (src, 0.5, 1.0, 0, dst, 8, 8, 8, ps, 4, pi),
               (src, 0.5, 1.0, 1, dst, 0, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 8, 0, 8, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 8, 8, 0, ps, 4, pi),
               (src, 0.5, 1.0, 1, dst, 9, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 8, 9, 8, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 8, 8, 9, ps, 4, pi),
               (src, 0.5, 1.0, 1, dst, 32769, 1, 1, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 1, 32769, 1, ps, 4, pi),
               (src, 0.5, 1.0, 1, dst, 1, 1, 32769, ps, 4, pi), (src, 0.5, 1.0, 1, dst, 32768, 32768, 2, ps, 4, pi),
               (src, 0.5, 1.0, 1, dst, 8, 8, 8, ps, 0, pi)]
        for args in bad:
            assert fn(*args) == 1, args
            assert b"f3d_label_components" in hip.f3d_last_error()
            if max(args[5:8]) > 32768 or args[5] * args[6] * args[7] > 2 ** 31 - 1:
                assert b"exceeds 32768 along an axis or 2^31 - 1 voxels" in hip.f3d_last_error()
        whole = box.download(dst, (8, 8, 8)).view(np.int32)
        assert (whole == LABEL_SENTINEL).all() and (sizes == SIZE_SENTINEL).all() and info.largest == 55     # a refused call writes nothing
        assert fn(src, 0.5, 1.0, 1, dst, 8, 8, 8, ps, 4, pi) == 0
        assert info.as_dict() == dict(foreground=512, background=0, nan=0, n_components=1, n_labels=1, dropped_components=0,
                                      dropped_voxels=0, largest=512)
        assert sizes.tolist() == [512] + [SIZE_SENTINEL] * 3 and (box.download(dst, (8, 8, 8)).view(np.int32) == 1).all()
        assert fn(src, 0.5, 1.0, 1, dst, 8, 8, 8, None, 0, pi) == 0       # a capacity of 0 goes with a null sizes
    finally:
        box.free()


# ---- Python, the driver, the command line ------------------------------------------------------------------------------------------------

def test_label_components_round_trips(f3d):
    volume, base = base_case((65, 5, 33), "noise-0.31")
    for min_voxels in (1, 5):
        got = f3d.label_components(volume, 0.5, 1.0, min_voxels)
        want = ref.apply_min_voxels(*base, min_voxels)
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, want[0])
        assert got.sizes.dtype == np.uint64 and np.array_equal(got.sizes, want[1])
        assert got.info == want[2] and got.n_labels == want[2]["n_labels"] == len(got)
    v = special_volume()
    got = f3d.label_components(v)                                       # the defaults: everything but the NaN is one mask
    want = ref.label_components(v, -INF, INF, 1)
    assert np.array_equal(got.labels, want[0]) and np.array_equal(got.sizes, want[1]) and got.info == want[2]
    none = f3d.label_components(v, 2.0, 3.0)
    assert none.n_labels == 0 and len(none.sizes) == 0 and not none.labels.any()


KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)


def test_segment_on_a_held_flow_feeds_label_motion_and_contacts(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    lo = float(np.quantile(f0, 0.9).astype(F32))
    want = ref.label_components(f0, lo, INF, 27)
    assert want[2]["n_labels"] > 3 and want[2]["dropped_components"] > 0
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        c = flow.segment(lo)                                            # min_voxels defaults to 27
        assert np.array_equal(c.labels, want[0]) and np.array_equal(c.sizes, want[1]) and c.info == want[2]
        kept = flow.label_motion(None, n_labels=c.n_labels)
        touching = flow.contacts(None, n_labels=c.n_labels, motion=kept["motion"])
        given = flow.label_motion(c.labels, n_labels=c.n_labels)        # the same calls with the downloaded labels passed explicitly
        explicit = flow.contacts(c.labels, n_labels=c.n_labels, motion=given["motion"])
        for name in "uvw":
            assert kept[name].tobytes() == given[name].tobytes()
        assert repr(kept["motion"].as_table()) == repr(given["motion"].as_table()) and kept["motion"].info == given["motion"].info
        assert touching.as_table() == explicit.as_table() and touching.info == explicit.info
        assert len(touching) == 0 and touching.info["surface"] > 0       # two components never share a face
        assert np.array_equal(flow.segment(lo, min_voxels=1).labels, ref.label_components(f0, lo, INF, 1)[0])
        assert np.array_equal(flow.segment(-INF, lo).labels, ref.label_components(f0, -INF, lo, 27)[0])
        flow.segment_end()
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), (u, v, ww)))
    finally:
        flow.destroy()


LINE = re.compile(r"bodies frame 0: (\d+) bodies of (\d+) foreground voxels \(largest (\d+)\), (\d+) bodies of (\d+) voxels dropped below (\d+), "
                  r"(\d+) background, (\d+) NaN")


def test_cli_segment_in_a_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([s0, s1, s0]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    lo = np.quantile(s0, 0.9).astype(F32)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    tail = ["--cumulative", "--label-motion", "rigid", "--contacts"]
    so = run("s", ["--segment", "%.9g:" % lo, "--segment-min-voxels", "9"] + tail)
    labels, sizes, info = ref.label_components(s0, lo, INF, 9)
    assert np.array_equal(np.fromfile(str(tmp_path / "s_0_labels.raw"), "<i4").reshape(d, h, w), labels)
    assert open(tmp_path / "s_0_bodies.csv").read().split() == ["label,voxels"] + [f"{i + 1},{s}" for i, s in enumerate(sizes.tolist())]
    (m,) = LINE.findall(so)
    assert [int(x) for x in m] == [info["n_labels"], info["foreground"], info["largest"], info["dropped_components"], info["dropped_voxels"],
                                   9, info["background"], info["nan"]]
    plain = run("p", ["--labels", str(tmp_path / "s_0_labels.raw")] + tail)
    assert not LINE.findall(plain)
    for k in range(2):
        names = [f"flow-{c}" for c in "uvw"] + [f"disp-{c}" for c in "uvw"] + [f"labelres-{c}" for c in "uvw"]
        for name in names:
            assert raw(f"s_{k}_{name}{suffix}") == raw(f"p_{k}_{name}{suffix}"), f"{name} of pair {k}"
        assert raw(f"s_{k}_labelmotion.csv") == raw(f"p_{k}_labelmotion.csv") and len(raw(f"s_{k}_labelmotion.csv").split(b"\n")) > 3
        assert raw(f"s_{k}_contacts.csv") == raw(f"p_{k}_contacts.csv")
    assert not any(n.startswith("p_") and ("bodies" in n or "labels.raw" in n) for n in os.listdir(tmp_path))
    # alone, with an upper bound only, on a single pair: the labels and the table, nothing that needs labels
    alone = subprocess.run(args[:-1] + ["--out", str(tmp_path / "a"), "--segment", ":%.9g" % lo], capture_output=True, text=True, timeout=300)
    assert alone.returncode == 0 and len(LINE.findall(alone.stdout)) == 1, alone.stdout[-2000:] + alone.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(tmp_path / "a_labels.raw"), "<i4").reshape(d, h, w), ref.label_components(s0, -INF, lo, 27)[0])
    assert not any("labelres" in n or "contacts" in n for n in os.listdir(tmp_path) if n.startswith("a_"))
