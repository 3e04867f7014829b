"""The grey-value histogram and the value range on the GPU: f3d_histogram and f3d_value_range against their numpy restatement
(tests/histogram_ref.py), never against themselves, in containers three columns, two rows and a plane larger than the box.  The float
padding of src holds a value INSIDE the range and the mask containers a non-zero sentinel outside the box, so a kernel that reads
padding miscounts; the counts array carries a sentinel behind its last bin.

Bounds.  Everything is an integer (or the bits of an input value) that is a function of the input alone: counts, every counter, min
and max equal the restatement byte for byte, and two calls give the same bytes.

Shapes: a wave covers 64 x, a workgroup 4 rows and 32 planes of a tile (csrc/f3d_histogram.hip), so 64 x 4 x 32 is exactly one tile,
65 x 5 x 33 one voxel past it along every axis, 130 x 9 x 70 has three tiles in x and z, and 160 x 96 x 72 = 216 tiles has many
workgroups flushing into the same accumulator.  Layouts: a constant volume (one run per wave), two values alternating along x (64 runs
of length one on two words), a ramp along x, noise, noise on three values (runs of random length), all NaN, and a crop of a real
frame.

The module's name makes it sort behind tests/test_gpu_pipeline.py, whose page-locked test is sensitive to what ran in the process
before it (LABBOOK.md); for the same reason the restatements of the table are computed by a child interpreter."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import histogram_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
COUNT_SENTINEL = 0x7F7F7F7F7F7F7F7F
SHAPES = [(1, 1, 1), (5, 3, 2), (64, 4, 32), (65, 5, 33), (130, 9, 70), (160, 96, 72)]        # (w, h, d)
LAYOUTS = ref.LAYOUTS + ("frame",)
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
INF = float("inf")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(w, h, d), layout -> (arrays, info) of ref.case_table: volumes, masks and the restated counts of every case, computed once by a
    child interpreter and read as read-only file mappings (this process builds and frees no block above 0.66 MB: histogram_ref.py)"""
    jobs = [[*dims, layout] for dims in SHAPES for layout in LAYOUTS]
    done = ref.in_child(jobs, str(tmp_path_factory.mktemp("histogram_cases")))
    return {(tuple(job[:3]), job[3]): case for job, case in zip(jobs, done)}


def case_volume(table, dims, layout):
    """(volume, lo, hi, padding byte) of a case of the table"""
    return (table[dims, layout][0]["volume"],) + ref.table_range(layout)


def bits_as_float(bits):
    return np.array([bits], np.uint32).view(F32)[0]


class Device:
    """a volume (and masks) in the corner of larger containers, with the entries called on the raw C ABI"""

    def __init__(self, f3d, volume, pad):
        d, h, w = volume.shape
        self.f3d, self.dims = f3d, (w, h, d)
        self.box = f3d.Containers(w + 3, h + 2, d + 1)
        self.src = self.box.alloc(fill=pad)
        self.box.upload(self.src, volume)
        self.box.set_current()

    def mask(self, mask):
        if mask is None:
            return 0
        ptr = self.box.alloc(fill=0x7F)                                 # outside the box every mask word lets a voxel through
        self.box.upload(ptr, np.ascontiguousarray(mask, np.int32).view(F32))
        return ptr

    def histogram(self, lo, hi, bins, mask=0):
        counts = np.full(bins + 3, COUNT_SENTINEL, np.uint64)
        info = self.f3d.HistogramInfo()
        self.f3d.check(self.f3d._histogram_entry()(self.src, mask, lo, hi, bins, *self.dims, counts.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                   C.byref(info)), "f3d_histogram")
        assert (counts[bins:] == COUNT_SENTINEL).all()
        return counts[:bins], info.as_dict()

    def value_range(self, mask=0):
        lo, hi, info = C.c_float(), C.c_float(), self.f3d.RangeInfo()
        self.f3d.check(self.f3d._value_range_entry()(self.src, mask, *self.dims, C.byref(lo), C.byref(hi), C.byref(info)), "f3d_value_range")
        return F32(lo.value), F32(hi.value), info.as_dict()

    def free(self):
        self.box.free()


def same_range(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


# ---- the table -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_counts_info_min_and_max_equal_the_restatement(f3d, table, dims, layout):
    arrays, infos = table[dims, layout]
    volume, (lo, hi, pad) = arrays["volume"], ref.table_range(layout)
    large = dims == SHAPES[-1] == ref.LARGE
    names, bin_counts = ref.table_plan(dims)
    assert len(names) * len(bin_counts) == (4 if large else 24)
    dev = Device(f3d, volume, pad)
    try:
        for name in names:
            ptr = dev.mask(arrays.get(f"mask_{name}"))
            low, high, counters = infos[f"range_{name}"]
            want_range = (bits_as_float(low), bits_as_float(high), counters)
            first, second = dev.value_range(ptr), dev.value_range(ptr)
            assert same_range(first, want_range) and same_range(second, want_range), (name, first, want_range)
            assert sum(first[2].values()) == volume.size
            for bins in bin_counts:
                want_counts, want_info = arrays[f"counts_{name}_{bins}"], infos[f"info_{name}_{bins}"]
                counts, info = dev.histogram(lo, hi, bins, ptr)
                again, info_again = dev.histogram(lo, hi, bins, ptr)
                assert info == want_info and counts.dtype == np.uint64 and np.array_equal(counts, want_counts), (name, bins, info, want_info)
                assert counts.tobytes() == again.tobytes() and info == info_again
                assert info["used"] + info["below"] + info["above"] + info["nan"] + info["masked"] == volume.size
                assert int(counts.sum()) == info["used"]
            if name == "zero":
                assert want_info["masked"] == volume.size and first[2]["finite"] == 0 and first[0] == INF and first[1] == -INF
    finally:
        dev.free()
    if layout == "nan":
        assert want_info["nan"] + want_info["masked"] == volume.size
    if layout == "constant" and not large:
        assert want_counts.max() == want_info["used"]                   # one bin holds everything


# ---- values --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def special_volume():
    w, h, d = 65, 5, 33
    rng = np.random.default_rng(4)
    v = rng.random((d, h, w)).astype(F32)
    one = F32(1)
    specials = np.array([np.nan, np.inf, -np.inf, 0.25, 0.75, np.nextafter(F32(0.25), -one), np.nextafter(F32(0.25), one),
                         np.nextafter(F32(0.75), -one), np.nextafter(F32(0.75), one), 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 0.5], F32)
    m = rng.random(v.shape) < 0.4
    v[m] = rng.choice(specials, size=int(m.sum()))
    v[10:14, 1:4, 20:40] = np.nan                                       # a NaN block, beside the NaN holes above
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("lo,hi", [(0.25, 0.75), (0.0, 0.5), (-1.0, 0.0), (-3e38, 3e-38), (0.75, 1.0), (-1e-37, 1e-37)], ids=str)
def test_special_values_and_bounds(f3d, lo, hi):
    """NaN holes and a NaN block, +-inf, values exactly lo and exactly hi and one ulp outside each, -0.0 with lo or hi = 0, denormals"""
    v = special_volume()
    dev = Device(f3d, v, 0x3F)
    try:
        for bins in (1, 7, 256, 4096):
            with np.errstate(over="ignore"):
                if not np.isfinite(ref.scale_of(lo, hi, bins)):
                    continue                                            # bins / (hi - lo) overflows: such a rule is refused (test_refusals)
            want = ref.histogram(v, lo, hi, bins)
            counts, info = dev.histogram(lo, hi, bins)
            assert info == want[1] and np.array_equal(counts, want[0]), (bins, info, want[1])
        if (lo, hi) == (0.25, 0.75):
            assert want[1]["nan"] == np.isnan(v).sum() > 80 and want[0][0] >= (v == F32(0.25)).sum() > 10 and want[0][-1] >= (v == F32(0.75)).sum() > 10
            assert want[1]["below"] >= (v == -INF).sum() + (v == np.nextafter(F32(0.25), F32(-1))).sum() > 20
        if (lo, hi) == (-1e-37, 1e-37):                                  # the last rule that was not refused: 7 bins
            assert want[1]["used"] == ((v == 0) | (np.abs(v) == F32(1e-45)) | (np.abs(v) == F32(1e-40))).sum() > 100
        got = dev.value_range()
        want_range = ref.value_range(v)
        assert same_range(got, want_range) and want_range[2]["infinite"] > 20 and got[0] == -1.0 * F32(1e-40)
    finally:
        dev.free()


@pytest.mark.parametrize("values,low,high", [((0.0, -0.0), -0.0, 0.0), ((-0.0, -0.0), -0.0, -0.0), ((0.0, 0.0), 0.0, 0.0),
                                             ((1e-45, 3e-45, 1e-40), 1e-45, 1e-40), ((-1e-45, 0.0, np.nan, np.inf), -1e-45, 0.0),
                                             ((-3.0e38, 3.0e38, -np.inf), -3.0e38, 3.0e38), ((np.nan, np.inf, -np.inf), np.inf, -np.inf)], ids=str)
def test_min_and_max_by_the_ordered_key(f3d, values, low, high):
    rng = np.random.default_rng(2)
    v = rng.choice(np.array(values, F32), size=(33, 5, 65))
    v[0, 0, :len(values)] = values                                     # every value occurs
    dev = Device(f3d, v, 0x3F)
    try:
        got = dev.value_range()
    finally:
        dev.free()
    assert same_range(got, ref.value_range(v))
    assert got[0].tobytes() == F32(low).tobytes() and got[1].tobytes() == F32(high).tobytes()


def test_nothing_is_carried_over_between_calls(f3d, table):
    """the accumulator and the counters are cleared per call: a large volume, then a small one of another shape and another range,
    then fewer bins than before"""
    big, lo, hi, pad = case_volume(table, (130, 9, 70), "noise")
    small = np.full((2, 3, 5), 0.5, F32)
    a = Device(f3d, big, pad)
    try:
        first = a.histogram(lo, hi, 4096)
        assert np.array_equal(first[0], table[(130, 9, 70), "noise"][0]["counts_none_4096"])
    finally:
        a.free()
    b = Device(f3d, small, 0x3F)
    try:
        counts, info = b.histogram(0.0, 1.0, 4096)
        assert info == dict(masked=0, nan=0, below=0, above=0, used=30) and counts[2048] == 30 and counts.sum() == 30
        counts, info = b.histogram(0.0, 1.0, 3)
        assert counts.tolist() == [0, 30, 0] and info["used"] == 30
        assert same_range(b.value_range(), ref.value_range(small))
    finally:
        b.free()


# ---- consistency with the labelling ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,bins", [("noise", 64), ("noise", 4096), ("frame", 256), ("noise-3", 7)])
def test_an_edge_as_threshold_selects_exactly_the_bins_above_it(f3d, table, layout, bins):
    volume, lo, hi, _ = case_volume(table, (65, 5, 33), layout)
    h = f3d.histogram(volume, bins=bins, range=(lo, hi))
    want = ref.histogram(volume, lo, hi, bins)
    assert np.array_equal(h.counts, want[0]) and h.info == want[1] and (h.lo, h.hi) == (lo, hi)
    for k in sorted({0, 1, bins // 3, bins // 2, bins - 1}):
        edge = h.edge(k)
        assert edge.tobytes() == ref.edge(lo, hi, bins, k).tobytes()
        upper = f3d.label_components(volume, lo=edge, hi=h.hi)
        assert upper.info["foreground"] == int(h.counts[k:].sum()), k
        if k:
            lower = f3d.label_components(volume, lo=h.lo, hi=np.nextafter(edge, F32(-INF)))
            assert lower.info["foreground"] == int(h.counts[:k].sum()), k
            assert upper.info["foreground"] + lower.info["foreground"] == h.info["used"]


def test_the_python_functions(f3d, table):
    volume, lo, hi, _ = case_volume(table, (65, 5, 33), "frame")
    found = f3d.value_range(volume)
    assert same_range(found, ref.value_range(volume))
    h = f3d.histogram(volume)                                          # 256 bins over the finite minimum and maximum
    assert (F32(h.lo), F32(h.hi)) == found[:2] and h.bins == 256
    want = ref.histogram(volume, found[0], found[1], 256)
    assert np.array_equal(h.counts, want[0]) and h.info == want[1]
    for classes in (2, 3):
        o, w = h.otsu(classes), ref.otsu(want[0], classes)
        assert (o.status, o.cuts.tolist(), o.populations.tolist(), o.objective) == w
        assert [v.tobytes() for v in o.values] == [ref.edge(h.lo, h.hi, 256, k).tobytes() for k in w[1]]
    assert h.rank(0) == ref.rank(want[0], 0) and h.quantile(0.5) == ref.rank(want[0], (volume.size - 1) // 2)
    mask = ref.masks(volume.shape)["half"]
    hm = f3d.histogram(volume, bins=64, range=(0.0, 255.0), mask=mask)
    wm = ref.histogram(volume, 0.0, 255.0, 64, mask)
    assert np.array_equal(hm.counts, wm[0]) and hm.info == wm[1] and same_range(f3d.value_range(volume, mask), ref.value_range(volume, mask))
    with pytest.raises(ValueError, match="constant"):
        f3d.histogram(np.full((2, 2, 2), 3.0, F32))
    with pytest.raises(ValueError, match="no finite voxel"):
        f3d.histogram(np.full((2, 2, 2), np.nan, F32))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals(f3d):
    hip = f3d.hip()
    fn, rn = f3d._histogram_entry(), f3d._value_range_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        src = box.new(np.full((8, 8, 8), 0.5, F32))
        box.set_current()
        counts = np.full(8, COUNT_SENTINEL, np.uint64)
        pc = counts.ctypes.data_as(C.POINTER(C.c_ulonglong))
        info = f3d.HistogramInfo()
        info.used = 55
        pi = C.byref(info)
        nan = float("nan")
        bad = [(0, 0, 0.0, 1.0, 4, 8, 8, 8, pc, pi), (src, 0, 0.0, 1.0, 4, 8, 8, 8, None, pi), (src, 0, 0.0, 1.0, 4, 8, 8, 8, pc, None),
               (src, 0, 1.0, 1.0, 4, 8, 8, 8, pc, pi), (src, 0, 1.0, 0.0, 4, 8, 8, 8, pc, pi), (src, 0, nan, 1.0, 4, 8, 8, 8, pc, pi),
               (src, 0, 0.0, nan, 4, 8, 8, 8, pc, pi), (src, 0, -INF, 1.0, 4, 8, 8, 8, pc, pi), (src, 0, 0.0, INF, 4, 8, 8, 8, pc, pi),
               (src, 0, -3e38, 3e38, 4, 8, 8, 8, pc, pi), (src, 0, 0.0, 1e-45, 4, 8, 8, 8, pc, pi),
               (src, 0, 0.0, 1.0, 0, 8, 8, 8, pc, pi), (src, 0, 0.0, 1.0, 4097, 8, 8, 8, pc, pi), (src, 0, 0.0, 1.0, 2 ** 40, 8, 8, 8, pc, pi),
               (src, 0, 0.0, 1.0, 4, 0, 8, 8, pc, pi), (src, 0, 0.0, 1.0, 4, 8, 0, 8, pc, pi), (src, 0, 0.0, 1.0, 4, 8, 8, 0, pc, pi),
               (src, 0, 0.0, 1.0, 4, 9, 8, 8, pc, pi), (src, 0, 0.0, 1.0, 4, 8, 9, 8, pc, pi), (src, 0, 0.0, 1.0, 4, 8, 8, 9, pc, pi),
               (src, 0, 0.0, 1.0, 4, 32769, 1, 1, pc, pi), (src, 0, 0.0, 1.0, 4, 32768, 32768, 9, pc, pi)]
        for args in bad:
            assert fn(*args) == 1, args
            assert b"f3d_histogram" in hip.f3d_last_error()
        assert (counts == COUNT_SENTINEL).all() and info.used == 55     # a refused call writes nothing
        lo, hi, rinfo = C.c_float(-7.0), C.c_float(-7.0), f3d.RangeInfo()
        rinfo.finite = 55
        pl, ph, pr = C.byref(lo), C.byref(hi), C.byref(rinfo)
        for args in [(0, 0, 8, 8, 8, pl, ph, pr), (src, 0, 8, 8, 8, None, ph, pr), (src, 0, 8, 8, 8, pl, None, pr), (src, 0, 8, 8, 8, pl, ph, None),
                     (src, 0, 0, 8, 8, pl, ph, pr), (src, 0, 8, 8, 9, pl, ph, pr), (src, 0, 1, 1, 32769, pl, ph, pr),
                     (src, 0, 32768, 32768, 9, pl, ph, pr)]:
            assert rn(*args) == 1, args
            assert b"f3d_value_range" in hip.f3d_last_error()
        assert lo.value == -7.0 and hi.value == -7.0 and rinfo.finite == 55
        assert fn(src, 0, 0.0, 1.0, 4, 8, 8, 8, pc, pi) == 0
        assert counts.tolist() == [0, 0, 512, 0] + [COUNT_SENTINEL] * 4 and info.as_dict() == dict(masked=0, nan=0, below=0, above=0, used=512)
        assert rn(src, 0, 8, 8, 8, pl, ph, pr) == 0 and (lo.value, hi.value, rinfo.finite) == (0.5, 0.5, 512)
    finally:
        box.free()


# ---- the driver and the command line ----------------------------------------------------------------------------------------------------

KW = dict(warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)


def test_the_driver_counts_the_frame_it_segments(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        got, free = flow.histogram(), f3d.histogram(f0)
        assert got.counts.tobytes() == free.counts.tobytes() and got.info == free.info and (got.lo, got.hi) == (free.lo, free.hi)
        want = ref.histogram(f0, *ref.value_range(f0)[:2], 256)
        assert np.array_equal(got.counts, want[0]) and got.info == want[1]
        got = flow.histogram(64, (0.25, 0.5))
        assert np.array_equal(got.counts, ref.histogram(f0, 0.25, 0.5, 64)[0]) and (got.lo, got.hi) == (0.25, 0.5)
        cut = free.otsu()
        by_token, by_value = flow.segment("otsu"), flow.segment(float(cut.values[0]))
        assert by_token.labels.tobytes() == by_value.labels.tobytes() and np.array_equal(by_token.sizes, by_value.sizes)
        assert by_token.info == by_value.info and by_token.info["foreground"] == int(cut.populations[1])
        three = f3d.histogram(f0, 64).otsu(3)
        middle = flow.segment("otsu1", "otsu2", min_voxels=1, bins=64)
        below = flow.segment(hi="otsu1", min_voxels=1, bins=64)
        above = flow.segment("otsu2", min_voxels=1, bins=64)
        assert [c.info["foreground"] for c in (below, middle, above)] == three.populations.tolist()
        assert not ((below.labels > 0) & (middle.labels > 0)).any() and not ((middle.labels > 0) & (above.labels > 0)).any()
        value = np.nextafter(three.values[1], F32(-INF))
        assert flow.segment(float(three.values[0]), float(value), min_voxels=1).labels.tobytes() == middle.labels.tobytes()
        flow.segment_end()
    finally:
        flow.destroy()


CUT = re.compile(r"threshold frame 0: otsu, 2 classes over (\d+) bins of \[(\S+), (\S+)\]: cut at bin (\d+) = (\S+) \((\d+) \| (\d+) voxels\), "
                 r"(\d+) NaN, (\d+) outside the range")
CUTS = re.compile(r"threshold frame 0: otsu, 3 classes over (\d+) bins of \[(\S+), (\S+)\]: cuts at bins (\d+), (\d+) = (\S+), (\S+) "
                  r"\((\d+) \| (\d+) \| (\d+) voxels\), (\d+) NaN, (\d+) outside the range")
COUNTED = re.compile(r"histogram frame 0: (\d+) bins of \[(\S+), (\S+)\]: (\d+) voxels counted, (\d+) NaN, (\d+) outside the range")


def test_cli_otsu_and_histogram(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([s0, s1]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    free = f3d.histogram(s0)
    cut = free.otsu()
    out = run("t", ["--segment", "otsu:", "--histogram"])
    (m,) = CUT.findall(out)
    assert [int(m[0]), int(m[3]), int(m[5]), int(m[6]), int(m[7]), int(m[8])] == [256, int(cut.cuts[0])] + cut.populations.tolist() + [0, 0]
    assert F32(m[1]) == F32(free.lo) and F32(m[2]) == F32(free.hi) and F32(m[4]).tobytes() == cut.values[0].tobytes()    # %.9g round-trips
    (c,) = COUNTED.findall(out)
    assert [int(c[0]), int(c[3]), int(c[4]), int(c[5])] == [256, s0.size, 0, 0]
    rows = [line.split(",") for line in open(tmp_path / "t_histogram.csv").read().split()]
    assert rows[0] == ["bin", "lower_edge", "count"] and [int(r[0]) for r in rows[1:]] == list(range(256))
    assert [int(r[2]) for r in rows[1:]] == free.counts.tolist()
    assert [F32(r[1]).tobytes() for r in rows[1:]] == [free.edge(k).tobytes() for k in range(256)]
    run("v", ["--segment", m[4] + ":"])                                # the printed cut, given as a number
    assert raw("t_labels.raw") == raw("v_labels.raw") and raw("t_bodies.csv") == raw("v_bodies.csv") and len(raw("t_bodies.csv").split()) > 2
    assert not os.path.exists(tmp_path / "v_histogram.csv")
    # three classes: the three phases are disjoint and add up to the counted voxels
    common = ["--segment-bins", "64", "--segment-min-voxels", "1"]
    phases = {}
    for tag, spec in (("lo", ":otsu1"), ("mid", "otsu1:otsu2"), ("hi", "otsu2:")):
        text = run(tag, ["--segment", spec] + common)
        (found,) = CUTS.findall(text)
        phases[tag] = np.fromfile(str(tmp_path / f"{tag}_labels.raw"), "<i4") > 0
    three = f3d.histogram(s0, 64).otsu(3)
    assert [int(x) for x in found[3:5]] == three.cuts.tolist() and [int(x) for x in found[7:10]] == three.populations.tolist()
    assert [int(p.sum()) for p in (phases["lo"], phases["mid"], phases["hi"])] == three.populations.tolist()
    assert not (phases["lo"] & phases["mid"]).any() and not (phases["mid"] & phases["hi"]).any() and not (phases["lo"] & phases["hi"]).any()
    assert int((phases["lo"] | phases["mid"] | phases["hi"]).sum()) == s0.size == int(free.info["used"])
    # --histogram alone, over a given range: the table and nothing that needs labels
    alone = run("a", ["--histogram", "--segment-bins", "16", "--segment-range", "0.25:0.5"])
    (c,) = COUNTED.findall(alone)
    want = ref.histogram(s0, 0.25, 0.5, 16)
    assert [int(c[0]), int(c[3]), int(c[4]), int(c[5])] == [16, want[1]["used"], 0, want[1]["below"] + want[1]["above"]]
    assert [int(line.split(",")[2]) for line in open(tmp_path / "a_histogram.csv").read().split()[1:]] == want[0].tolist()
    assert not any(n.startswith("a_") and ("labels" in n or "bodies" in n) for n in os.listdir(tmp_path))
    # a frame without a cut stops the run with a message that says which
    flat = str(tmp_path / "flat.raw")
    np.full((d, h, w), 0.5, F32).tofile(flat)
    r = subprocess.run(args[:-2] + [flat, paths[1], "--out", str(tmp_path / "c"), "--segment", "otsu:"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "the frame is constant" in r.stdout, r.stdout[-2000:]
    two = np.where(np.arange(w) < w // 2, F32(0.25), F32(0.75)) * np.ones((d, h, w), F32)
    two.astype(F32).tofile(flat)
    r = subprocess.run(args[:-2] + [flat, paths[1], "--out", str(tmp_path / "c"), "--segment", "otsu1:"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "fewer than 3 of the 256 bins" in r.stdout, r.stdout[-2000:]
    assert not any(n.startswith("c_") and ("labels" in n or "bodies" in n) for n in os.listdir(tmp_path))
