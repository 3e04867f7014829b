"""Bodies of a thresholded volume with touching bodies taken apart, on the GPU: f3d_split_components against its numpy restatement
(tests/nearest_ref.py on top of tests/components_ref.py), never against itself, in containers three columns, two rows and a plane
larger than the box, the float padding of src filled with a FOREGROUND value and labels_out with a sentinel that must survive outside
the box.  Beyond 65 x 5 x 33 the restatement runs once per module in a child interpreter and is read back as file mappings:
tests/nearest_ref.py says why this process must not build and free its large blocks.

Bounds.  Everything is an integer function of the input: labels_out, sizes and every counter of the info equal the restatement bit for
bit; with core_d2 = 1 they equal f3d_label_components' on the same input.

Shapes: the passes are those of test_gpu_components.py and test_gpu_nearest.py and are tested there on their own; here 65 x 5 x 33 (one
voxel past a tile and past a wave's step along every axis) carries the identity, and the packing of 18 overlapping spheres in
56 x 48 x 40, which thresholds to ONE component, carries the split."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cref
import nearest_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SENTINEL = 0x7F
LABEL_SENTINEL = 0x7F7F7F7F
SIZE_SENTINEL = 0x7F7F7F7F7F7F7F7F
INF = float("inf")


def device_split(f3d, volume, lo, hi, core_d2, min_voxels, capacity=None, keep_sizes=True, entry=None):
    """f3d_split_components (or, with entry="components", f3d_label_components) on a box in the corner of larger containers:
    (labels, sizes array with its tail, info dict, the whole label container)"""
    d, h, w = volume.shape
    box = f3d.Containers(w + 3, h + 2, d + 1)
    room = min(volume.size, 16384) if capacity is None else capacity   # no case here has more classes; the array stays small
    try:
        src = box.alloc(fill=0x3F)                                       # 0x3F3F3F3F is 0.747: foreground of every range used here
        box.upload(src, volume)
        box.set_current()
        dst = box.alloc(fill=SENTINEL)
        sizes = np.full(room + 3, SIZE_SENTINEL, np.uint64)
        ptr = sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)) if keep_sizes else None
        if entry == "components":
            info = f3d.ComponentInfo()
            f3d.check(f3d._components_entry()(src, lo, hi, min_voxels, dst, w, h, d, ptr, room if keep_sizes else 0, C.byref(info)),
                      "f3d_label_components")
        else:
            info = f3d.SplitInfo()
            f3d.check(f3d._split_entry()(src, lo, hi, core_d2, min_voxels, dst, w, h, d, ptr, room if keep_sizes else 0, C.byref(info)),
                      "f3d_split_components")
        whole = box.download(dst, (w + 3, h + 2, d + 1)).view(np.int32)
    finally:
        box.free()
    return whole[:d, :h, :w].copy(), sizes, info.as_dict(), whole


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
    assert info["n_components"] == info["n_cores"] + info["remainder_bodies"] == info["n_labels"] + info["dropped_components"]


JOBS = [("packing", 49, 1), ("packing", 36, 1), ("packing", 64, 1), ("packing", 82, 1), ("packing", 2 ** 31 - 1, 1), ("packing", 2 ** 40, 1),
        ("packing", 43, 1), ("packing", 49, 2742), ("frames", 49, 27), ("necked", 16, 1), ("necked", 16, 33), ("necked", 16, 34),
        ("necked", 16, 2 ** 63), ("noise-nan", 2, 1), ("noise-nan", 2, 4), ("box", 2 ** 31 - 1, 1), ("box", 2 ** 31, 1)]
EXTRA = ("contacts", "plain_components")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{(volume name, core_d2, min_voxels): (volume, (labels, sizes, info), extra, arrays)}: the restatement of every split this module
    asks for beyond 65 x 5 x 33, computed once by a child interpreter (tests/nearest_ref.py says why), shared as read-only file mappings
    and left unchanged.  extra: the contacts between the resulting bodies and the components of the unsplit foreground"""
    got = ref.in_child([("split", list(job)) for job in JOBS], str(tmp_path_factory.mktemp("split")))
    out = {}
    for job, (a, info) in zip(JOBS, got):
        extra = {k: info.pop(k) for k in EXTRA}
        out[job] = (a["volume"], (a["labels"], a["sizes"], info), extra, a)
    return out


@pytest.mark.parametrize("layout", cref.LAYOUTS)
def test_core_d2_of_one_is_label_components_bit_for_bit(f3d, layout):
    mask = cref.layout_mask(layout, (33, 5, 65))
    volume = cref.as_volume(mask, 0.75, 0.25)
    for min_voxels in (1, 3):
        labels, sizes, info, whole = device_split(f3d, volume, 0.5, 1.0, 1, min_voxels)
        plain = device_split(f3d, volume, 0.5, 1.0, None, min_voxels, entry="components")
        assert whole.tobytes() == plain[3].tobytes() and sizes.tobytes() == plain[1].tobytes()
        assert {k: info[k] for k in cref.INFO} == plain[2]
        want = cref.label_components(volume, 0.5, 1.0, min_voxels)      # and both are the restatement's
        assert np.array_equal(labels, want[0]) and {k: info[k] for k in cref.INFO} == want[2]
        every = cref.label_components(volume, 0.5, 1.0, 1)[2]
        assert info["connected_components"] == info["n_cores"] == every["n_components"] and info["core_voxels"] == info["foreground"]
        assert info["remainder_bodies"] == info["remainder_voxels"] == 0


def test_the_sphere_packing_is_one_component_and_splits_into_its_spheres(f3d, cases):
    volume, want, extra, _ = cases["packing", 49, 1]
    assert volume.shape == (40, 48, 56) and extra["plain_components"] == 1
    assert want[2]["n_labels"] == 18 and want[2]["remainder_voxels"] == 0 and want[2]["connected_components"] == 1
    assert want[1].min() > 2600 and extra["contacts"] >= 31
    first = device_split(f3d, volume, 0.5, 1.0, 49, 1)
    check_call(first, want, volume.shape)
    second = device_split(f3d, volume, 0.5, 1.0, 49, 1)
    assert first[3].tobytes() == second[3].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]


@pytest.mark.parametrize("core_d2", [36, 64, 82, 2 ** 31 - 1, 2 ** 40])
def test_the_packing_at_other_core_sizes(f3d, cases, core_d2):
    """82 is above every depth of a sphere of radius 9: no core, every voxel in the one remainder; so is anything larger"""
    volume, want, _, _ = cases["packing", core_d2, 1]
    if core_d2 >= 82:
        assert want[2]["n_cores"] == 0 and want[2]["remainder_bodies"] == 1 and want[2]["remainder_voxels"] == want[2]["foreground"]
    else:
        assert want[2]["n_labels"] == 18
    check_call(device_split(f3d, volume, 0.5, 1.0, core_d2, 1), want, volume.shape)


def test_a_whole_box_of_foreground_is_all_core(f3d, cases):
    volume, want, _, _ = cases["box", 2 ** 31 - 1, 1]
    assert want[2]["core_voxels"] == 210 and want[2]["n_labels"] == 1
    check_call(device_split(f3d, volume, 0.5, 1.0, 2 ** 31 - 1, 1), want, volume.shape)
    volume, none, _, _ = cases["box", 2 ** 31, 1]                        # no voxel is that deep: one remainder
    assert none[2]["core_voxels"] == 0 and none[2]["remainder_bodies"] == 1
    check_call(device_split(f3d, volume, 0.5, 1.0, 2 ** 31, 1), none, volume.shape)


def test_two_balls_and_a_neck_and_a_coreless_ball_behind_one_plane_of_background(f3d, cases):
    volume, want, _, arrays = cases["necked", 16, 1]
    small = arrays["small"]
    assert want[2]["connected_components"] == 2 and want[2]["n_cores"] == 2 and want[2]["remainder_bodies"] == 1
    assert want[2]["n_labels"] == 3 and want[2]["remainder_voxels"] == small.sum() == want[1][2] == 33
    assert (want[0][small] == 3).all() and not (want[0][~small] == 3).any()     # the nearest core is the other component's: a label of its own
    check_call(device_split(f3d, volume, 0.5, 1.0, 16, 1), want, volume.shape)
    # min_voxels exactly a class size and one above
    at, above = cases["necked", 16, 33][1], cases["necked", 16, 34][1]
    assert at[2]["n_labels"] == 3 and above[2]["n_labels"] == 2 and above[2]["dropped_voxels"] == 33
    check_call(device_split(f3d, volume, 0.5, 1.0, 16, 33), at, volume.shape)
    check_call(device_split(f3d, volume, 0.5, 1.0, 16, 34), above, volume.shape)
    check_call(device_split(f3d, volume, 0.5, 1.0, 16, 2 ** 63), cases["necked", 16, 2 ** 63][1], volume.shape)


def test_nan_voxels_noise_and_remainders(f3d, cases):
    """noise at 0.6 with NaN holes at core_d2 = 2: many small cores, many components without one"""
    volume, want, _, _ = cases["noise-nan", 2, 1]
    assert want[2]["n_cores"] > 5 and want[2]["remainder_bodies"] > 5 and want[2]["nan"] > 50
    check_call(device_split(f3d, volume, 0.5, 1.0, 2, 1), want, volume.shape)
    check_call(device_split(f3d, volume, 0.5, 1.0, 2, 4), cases["noise-nan", 2, 4][1], volume.shape)


def test_the_capacity_of_sizes(f3d, cases):
    volume, want, _, _ = cases["packing", 49, 1]
    for capacity in (18, 14, 1, 23):
        labels, sizes, info, whole = device_split(f3d, volume, 0.5, 1.0, 49, 1, capacity=capacity)
        k = min(18, capacity)
        assert info == want[2] and np.array_equal(labels, want[0])
        assert np.array_equal(sizes[:k], want[1][:k]) and (sizes[k:] == SIZE_SENTINEL).all()
    labels, sizes, info, whole = device_split(f3d, volume, 0.5, 1.0, 49, 1, keep_sizes=False)
    assert info == want[2] and np.array_equal(labels, want[0]) and (sizes == SIZE_SENTINEL).all()


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._split_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        src = box.new(np.full((8, 8, 8), 0.75, F32))
        dst = box.alloc(fill=SENTINEL)
        box.set_current()
        sizes = np.full(4, SIZE_SENTINEL, np.uint64)
        ps = sizes.ctypes.data_as(C.POINTER(C.c_ulonglong))
        info = f3d.SplitInfo()
        info.largest = 55
        pi = C.byref(info)
        nan = float("nan")
        bad = [(0, 0.5, 1.0, 4, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 4, 1, 0, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 8, 8, 8, ps, 4, None),
               (src, 0.5, 1.0, 4, 1, src, 8, 8, 8, ps, 4, pi), (src, nan, 1.0, 4, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, nan, 4, 1, dst, 8, 8, 8, ps, 4, pi),
               (src, 1.0, 0.5, 4, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 0, 1, dst, 8, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 4, 0, dst, 8, 8, 8, ps, 4, pi),
               (src, 0.5, 1.0, 4, 1, dst, 0, 8, 8, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 8, 8, 0, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 9, 8, 8, ps, 4, pi),
               (src, 0.5, 1.0, 4, 1, dst, 8, 9, 8, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 8, 8, 9, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 32769, 1, 1, ps, 4, pi),
               (src, 0.5, 1.0, 4, 1, dst, 32768, 32768, 1, ps, 4, pi), (src, 0.5, 1.0, 4, 1, dst, 8, 8, 8, ps, 0, pi)]
        for args in bad:
            assert fn(*args) == 1, args
            assert b"f3d_split_components" in hip.f3d_last_error()
        assert b"capacity of 0" in hip.f3d_last_error()
        whole = box.download(dst, (8, 8, 8)).view(np.int32)
        assert (whole == LABEL_SENTINEL).all() and (sizes == SIZE_SENTINEL).all() and info.largest == 55     # a refused call writes nothing
        assert fn(src, 0.5, 1.0, 4, 1, dst, 8, 8, 8, ps, 4, pi) == 0
        assert info.as_dict() == dict(foreground=512, background=0, nan=0, n_components=1, n_labels=1, dropped_components=0, dropped_voxels=0,
                                      largest=512, connected_components=1, core_voxels=512, n_cores=1, remainder_bodies=0, remainder_voxels=0)
        assert sizes.tolist() == [512] + [SIZE_SENTINEL] * 3 and (box.download(dst, (8, 8, 8)).view(np.int32) == 1).all()
    finally:
        box.free()


# ---- Python, the driver, the command line ------------------------------------------------------------------------------------------------

def test_python_split_components(f3d, cases):
    volume, want, _, _ = cases["packing", 49, 1]
    got = f3d.split_components(volume, 0.5, 1.0, core_d2=49)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, want[0]) and np.array_equal(got.sizes, want[1])
    assert got.info == want[2] and got.n_labels == 18 == len(got)
    by_radius = f3d.split_components(volume, 0.5, 1.0, radius=6.5)       # ceil(42.25) = 43
    w43 = cases["packing", 43, 1][1]
    assert np.array_equal(by_radius.labels, w43[0]) and by_radius.info == w43[2]
    assert int(want[1].min()) == 2741                                    # one above the smallest body
    few, fewer = f3d.split_components(volume, 0.5, 1.0, core_d2=49, min_voxels=2742), cases["packing", 49, 2742][1]
    assert few.n_labels == 17 and few.info == fewer[2] and np.array_equal(few.labels, fewer[0]) and np.array_equal(few.sizes, fewer[1])


KW = dict(warp_levels_count=4, outer_iterations_count=3, inner_iterations_count=3)


def test_segment_with_a_split_feeds_label_motion_and_contacts(f3d, cases):
    f0, want, extra, _ = cases["frames", 49, 27]
    f1 = np.roll(f0, 1, axis=2)
    d, h, w = f0.shape
    assert want[2]["n_labels"] == 18
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        c = flow.segment(0.5, split=49)
        assert np.array_equal(c.labels, want[0]) and np.array_equal(c.sizes, want[1]) and c.info == want[2]
        kept = flow.label_motion(None, n_labels=c.n_labels)
        touching = flow.contacts(None, n_labels=c.n_labels, motion=kept["motion"])
        assert len(touching) == extra["contacts"] >= 31                  # the table is no longer empty
        explicit = flow.contacts(c.labels, n_labels=c.n_labels, motion=kept["motion"])
        assert touching.as_table() == explicit.as_table()
        plain = flow.segment(0.5)                                         # split=None is the call as it was
        assert plain.n_labels == 1 and "n_cores" not in plain.info
        flow.segment_end()
    finally:
        flow.destroy()


SPLIT_LINE = re.compile(r"split at d2 >= (\d+): (\d+) components, (\d+) cores, (\d+) remainder bodies of (\d+) voxels")


def test_cli_segment_split_equals_a_run_on_the_labels_from_python(f3d, cases, tmp_path):
    f0, want, _, _ = cases["frames", 49, 27]
    f1 = np.roll(f0, 1, axis=2)
    d, h, w = f0.shape
    paths = []
    for i, f in enumerate([f0, f1]):
        p = str(tmp_path / f"f{i}.raw")
        np.asarray(f).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    tail = ["--label-motion", "rigid", "--contacts"]
    so = run("s", ["--segment", "0.5:", "--segment-split-d2", "49"] + tail)
    got = f3d.split_components(f0, 0.5, INF, core_d2=49, min_voxels=27)
    assert np.array_equal(got.labels, want[0])
    assert np.array_equal(np.fromfile(str(tmp_path / "s_labels.raw"), "<i4").reshape(d, h, w), got.labels)
    assert open(tmp_path / "s_bodies.csv").read().split() == ["label,voxels"] + [f"{i + 1},{s}" for i, s in enumerate(got.sizes.tolist())]
    (m,) = SPLIT_LINE.findall(so)
    assert [int(x) for x in m] == [49, 1, 18, 0, 0]
    labels_file = tmp_path / "from_python.raw"
    got.labels.astype("<i4").tofile(labels_file)
    plain = run("p", ["--labels", str(labels_file)] + tail)
    assert not SPLIT_LINE.findall(plain)
    for name in [f"flow-{c}" for c in "uvw"] + [f"labelres-{c}" for c in "uvw"]:
        assert raw(f"s_{name}{suffix}") == raw(f"p_{name}{suffix}"), name
    assert raw("s_labelmotion.csv") == raw("p_labelmotion.csv") and len(raw("s_labelmotion.csv").split(b"\n")) > 18
    assert raw("s_contacts.csv") == raw("p_contacts.csv") and len(raw("s_contacts.csv").split(b"\n")) > 31
    by_radius = run("r", ["--segment", "0.5:", "--segment-split", "7"])  # ceil(49) = 49: the same labels
    assert raw("r_labels.raw") == raw("s_labels.raw") and SPLIT_LINE.findall(by_radius)[0][0] == "49"
