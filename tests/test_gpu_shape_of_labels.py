"""The shape sums of labelled bodies on the GPU: f3d_label_shape_sums against its numpy restatement (tests/label_shape_ref.py), never
against itself, all 36 words of every label and the info bit for bit; two independent kernels as cross-checks (the coordinate moments
of f3d_label_motion_sums, the face classes of f3d_label_contacts); the refusals; label_shapes, OpticalFlow.label_shapes after segment()
before any solve; and bin/flow3d --label-shape in a short sequence whose other outputs stay byte for byte the same.

Bounds.  Every word is an exact integer: equality, whatever the schedule, and two calls give the same bytes.

Shapes.  The kernel's tile is 64 x 4 x 32 (a wave covers 64 x, a workgroup 4 rows, a run 32 planes): 64x4x32 is exactly one tile,
65x5x33 one voxel more along every axis, so every seam and every diagonal across a seam, an edge and a corner of a tile occurs;
130x9x70 has three tiles along x and z; 1x1x1, 2x2x2 and 3x70x2 are thinner than the neighbourhood.  The LDS table has 128 slots: the
1000 random labels overflow it in every full tile, so runs go straight to the global rows.

Padding.  The box lies in the corner of a container three columns, two rows and a plane larger whose padding voxels all carry a VALID
label that also occurs on the far faces of the box: a kernel that reads a neighbour outside the box counts pairs, squares and cubes
that are not there.  The bytes between the container's width and its pitch are 0xFF.

Host memory and the module's name.  The name makes it sort behind tests/test_gpu_pipeline.py, whose page-locked test is sensitive to
what ran in the process before it (LABBOOK.md): with this module in front of it, under the name tests/test_gpu_label_shape.py, that
test met HIP error 700 in two whole-suite runs of three.  For the same reason the restatement runs in a child interpreter, once for
all cases, the tests read its label volumes, containers and sums as read-only file mappings, and what a test of this module allocates
itself stays below 0.5 MB."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import label_shape_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SENTINEL = 0x7F
SHAPES = [(1, 1, 1), (2, 2, 2), (64, 4, 32), (65, 5, 33), (3, 70, 2), (130, 9, 70)]
LAYOUTS = ("one", "voronoi", "random", "checker", "spare", "outside", "cross")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(dims, layout) -> (labels, container, n_labels, the restatement's sums and info): every case computed once, by a child interpreter,
    and read as read-only file mappings (label_shape_ref.in_child says why)"""
    keys = [(dims, layout) for dims in SHAPES for layout in LAYOUTS]
    made = ref.in_child([[list(dims), layout] for dims, layout in keys], str(tmp_path_factory.mktemp("label_shape_cases")))
    out = {}
    for key, (arrays, info) in zip(keys, made):
        n_labels = info.pop("n_labels")
        out[key] = (arrays["labels"], arrays["container"], n_labels, arrays["sums"], info)
    return out


def device_sums(f3d, container, dims, n_labels, calls=1, info=True):
    """f3d_label_shape_sums on the box `dims` in the corner of `container`, whose padding carries a body's label: (structured array over
    the rows, info dict) per call; the rows are filled with the sentinel byte before every call"""
    w, h, d = dims
    fn = f3d._label_shape_entry()
    dc, hc, wc = container.shape
    box = f3d.Containers(wc, hc, dc)
    try:
        pl = box.new(container.view(F32))
        box.set_current()
        out = []
        for _ in range(calls):
            rows, counted = (f3d.LabelShapeSums * n_labels)(), f3d.LabelShapeInfo()
            C.memset(rows, SENTINEL, C.sizeof(rows))
            f3d.check(fn(pl, n_labels, w, h, d, rows, C.byref(counted) if info else None), "f3d_label_shape_sums")
            out.append((np.frombuffer(rows, ref.SUMS_DTYPE), counted.as_dict()))          # a view, not a copy
    finally:
        box.free()
    return out if calls > 1 else out[0]


def check_sums(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() == want.tobytes():
        return
    for name in ref.SUMS_DTYPE.names:                                    # say which word of which label differs
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, (name, "label", int(bad[0][0]) + 1, got[name][bad[0][0]].tolist(), want[name][bad[0][0]].tolist())


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_sums_equal_the_restatement_bit_for_bit(f3d, cases, dims, layout):
    labels, container, n_labels, want, info_want = cases[dims, layout]
    (first, info), (second, info2) = device_sums(f3d, container, dims, n_labels, calls=2)
    assert first.tobytes() == second.tobytes() and info == info2        # two calls, identical bytes
    assert info == info_want
    check_sums(first, want)
    w, h, d = dims
    assert sum(info.values()) == w * h * d and int(first["n"].sum()) == info["labelled"]
    if w * h * d > 100:
        assert (info["foreign"] > 0 and info["background"] > 0) == (layout == "outside")
        if layout == "one":
            assert first["border"][0].tolist() == [2 * h * d, 2 * w * d, 2 * w * h] and int(first["cubes"][0]) == (w - 1) * (h - 1) * (d - 1)
        if layout == "checker":
            assert not first["pairs"][:, :3].any() and first["pairs"][:, 3:9].all() and not first["pairs"][:, 9:].any()
        if layout == "spare":
            assert (first["n"][40:] == 0).all() and (first["hi"][40:] == -1).all() and (first["lo"][40:] == 0).all()
        if layout == "cross":
            assert (first["border"][40] > 0).all() and first["lo"][40].tolist() == [0, 0, 0] and first["hi"][40].tolist() == [w - 1, h - 1, d - 1]
        if layout == "random" and dims == (130, 9, 70):
            assert (first["n"] > 0).all()


def test_the_info_is_optional(f3d, cases):
    dims = (65, 5, 33)
    _, container, n_labels, want, _ = cases[dims, "voronoi"]
    got, _ = device_sums(f3d, container, dims, n_labels, info=False)
    check_sums(got, want)


# ---- cross-checks against independent kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["voronoi", "outside"])
def test_the_moments_are_those_of_label_motion_sums(f3d, cases, layout):
    """with a finite displacement everywhere f3d_label_motion_sums counts every voxel of a label, in doubled coordinates about the
    centre: x2 = 2 x - (N - 1), so sum x2 = 2 s1 - (N - 1) n and sum x2_i x2_k = 4 s2_ik - 2 (N_k - 1) s1_i - 2 (N_i - 1) s1_k + (N_i - 1)(N_k - 1) n"""
    dims = (65, 5, 33)
    labels, container, n_labels, _, _ = cases[dims, layout]
    got, info = device_sums(f3d, container, dims, n_labels)
    zero = np.zeros(labels.shape, F32)
    sums, motion_info = f3d.label_motion_sums(zero, zero, zero, labels, n_labels)
    assert motion_info["used"] == info["labelled"] and motion_info["background"] == info["background"] and motion_info["foreign"] == info["foreign"]
    N = [k - 1 for k in dims]
    for L in range(n_labels):
        n, s1, s2 = int(got["n"][L]), [int(v) for v in got["s1"][L]], [int(v) for v in got["s2"][L]]
        assert sums[L].n == n
        assert [2 * v for v in sums[L].Sx] == [2 * s1[i] - N[i] * n for i in range(3)]
        assert [4 * v for v in sums[L].Sxx] == [4 * s2[j] - 2 * N[k] * s1[i] - 2 * N[i] * s1[k] + N[i] * N[k] * n for j, (i, k) in enumerate(ref.S2)]


@pytest.mark.parametrize("layout", ["voronoi", "checker", "cross"])
def test_the_open_faces_are_those_of_label_contacts(f3d, cases, layout):
    """without foreign labels an open end of a body along an axis is the box border, a face to the background (one end) or a contact face
    (one end of each body)"""
    dims = (65, 5, 33)
    w, h, d = dims
    labels, container, n_labels, _, _ = cases[dims, layout]
    labels = np.array(labels)
    labels[labels % 5 == 0] = 0                                           # some background
    container = np.array(container)
    container[:d, :h, :w] = labels
    got, _ = device_sums(f3d, container, dims, n_labels)
    contacts = f3d.label_contacts(None, None, None, labels, n_labels)
    assert contacts.info["foreign"] == 0 and contacts.info["complete"] == 1
    ends = sum(2 * (int(got["n"][L]) - int(got["pairs"][L, k])) - int(got["border"][L, k]) for L in range(n_labels) for k in range(3))
    assert ends == contacts.info["surface"] + 2 * contacts.info["contact"] > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._label_shape_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        lab = box.new(np.ones((8, 8, 8), np.int32).view(F32))
        box.set_current()
        rows, info = (f3d.LabelShapeSums * 2)(), f3d.LabelShapeInfo()
        C.memset(rows, SENTINEL, C.sizeof(rows))
        info.labelled = 55
        tail = (rows, C.byref(info))
        bad = [(0, 2, 8, 8, 8, *tail), (lab, 2, 8, 8, 8, None, C.byref(info)), (lab, 0, 8, 8, 8, *tail), (lab, (1 << 22) + 1, 8, 8, 8, *tail),
               (lab, 2, 0, 8, 8, *tail), (lab, 2, 8, 0, 8, *tail), (lab, 2, 8, 8, 0, *tail),
               (lab, 2, 9, 8, 8, *tail), (lab, 2, 8, 9, 8, *tail), (lab, 2, 8, 8, 9, *tail),          # larger than the container
               (lab, 2, 32769, 1, 1, *tail), (lab, 2, 1, 32769, 1, *tail), (lab, 2, 1, 1, 32769, *tail), (lab, 2, 32768, 32768, 2, *tail)]
        for args in bad:
            assert fn(*args) != 0, args
            assert b"f3d_label_shape_sums" in hip.f3d_last_error()
            if max(args[2:5]) > 32768 or args[2] * args[3] * args[4] > 2 ** 31 - 1:
                assert b"exceeds 32768 along an axis or 2^31 - 1 voxels" in hip.f3d_last_error()
        raw = np.frombuffer(rows, np.uint8)
        assert raw.min() == SENTINEL == raw.max() and info.labelled == 55   # a refused call writes nothing
        assert fn(lab, 2, 8, 8, 8, *tail) == 0 and info.labelled == 512 and rows[0].n == 512 and rows[1].n == 0
        assert list(rows[0].lo) == [0, 0, 0] and list(rows[0].hi) == [7, 7, 7] and list(rows[1].hi) == [-1, -1, -1]
        assert fn(lab, 1, 7, 6, 5, *tail) == 0 and rows[0].n == 210 and rows[0].cubes == 6 * 5 * 4      # a box smaller than the container
    finally:
        box.free()


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------------

def test_label_shapes_from_anywhere(f3d, cases):
    labels, _, n_labels, want, info_want = cases[(65, 5, 33), "outside"]
    sums, info = f3d.label_shape_sums(labels, n_labels)
    check_sums(sums, want)
    assert info == info_want
    shapes = f3d.label_shapes(labels, n_labels)
    solved = f3d.solve_label_shapes(want)
    assert shapes.rows.tobytes() == solved.rows.tobytes() and shapes.info == info_want
    assert len(shapes) == n_labels and shapes.voxels.tolist() == want["n"].tolist()
    assert shapes.as_table()[3]["euler"] == ref.euler(want[3])
    with pytest.raises(ValueError, match="n_labels"):
        f3d.label_shapes(labels)                                          # n_labels None is labels.max(): here a foreign 2^31 - 1


def test_shapes_of_the_segmented_frame_before_any_solve(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        with pytest.raises(ValueError, match="n_labels"):                  # nothing segmented, no number given
            flow.label_shapes()
        with pytest.raises(f3d.F3dError, match="labels"):                  # nothing on the device yet
            flow.label_shapes(None, n_labels=3)
        flow.upload(f0, f1)
        bodies = flow.segment(lo="otsu", min_voxels=8)
        assert bodies.n_labels > 3
        shapes = flow.label_shapes()                                       # the labels segment() left on the device
        anywhere = f3d.label_shapes(bodies.labels, bodies.n_labels)        # which the tests above hold to the restatement
        assert shapes.rows.tobytes() == anywhere.rows.tobytes() and shapes.info == anywhere.info
        assert shapes.info["labelled"] == int(bodies.sizes.sum())
        assert shapes.voxels.tolist() == bodies.sizes.tolist() and (shapes.status == 0).all()
        mine = np.where(bodies.labels == 2, 1, 0).astype(np.int32)
        given = flow.label_shapes(mine)                                    # labels from the caller replace them
        assert len(given) == 1 and given.voxels[0] == bodies.sizes[1] and given.box[0].tolist() == shapes.box[1].tolist()
        assert given.rows.tobytes() == flow.label_shapes(None, n_labels=1).rows.tobytes()
        with pytest.raises(ValueError):
            flow.label_shapes(mine[:, :, :-1])
        flow.segment_end()
    finally:
        flow.destroy()


# ---- bin/flow3d --label-shape ------------------------------------------------------------------------------------------------------------------

LINE = re.compile(r"shapes frame 0: (\d+) bodies, (\d+) empty, (\d+) touch the border, median diameter (\S+), median sphericity (\S+), "
                  r"(\d+) with Euler number != 1")
HEADER = ("label,status,voxels,x_lo,y_lo,z_lo,x_hi,y_hi,z_hi,border_x,border_y,border_z,centroid_x,centroid_y,centroid_z,diameter,"
          "semi_axis_1,semi_axis_2,semi_axis_3,axis_1_x,axis_1_y,axis_1_z,axis_2_x,axis_2_y,axis_2_z,axis_3_x,axis_3_y,axis_3_z,faces,"
          "surface,sphericity,euler")


def check_table(f3d, path, line, labels, n_labels):
    """<tag>_shapes.csv and the line that sums it up against label_shapes of the same labels"""
    shapes = f3d.label_shapes(labels, n_labels)
    rows = open(path).read().strip().split("\n")
    assert rows[0] == HEADER and len(rows) == 1 + n_labels
    for i, row in enumerate(rows[1:]):
        cells = row.split(",")
        assert len(cells) == 32
        assert [int(c) for c in cells[:12]] == [i + 1, shapes.status[i], shapes.voxels[i], *shapes.box[i].ravel().tolist(),
                                                *shapes.border[i].tolist()]
        exp = np.concatenate([shapes.centroid[i], [shapes.diameter[i]], shapes.semi_axes[i], shapes.axes[i].ravel()])
        assert np.allclose([float(c) for c in cells[12:28]], exp, rtol=1e-8, atol=1e-12, equal_nan=True)
        assert int(cells[28]) == shapes.faces[i] and int(cells[31]) == shapes.euler[i]
        assert np.allclose([float(cells[29]), float(cells[30])], [shapes.surface[i], shapes.sphericity[i]], rtol=1e-8, equal_nan=True)
    ok = shapes.status == 0
    assert [int(line[k]) for k in (0, 1, 2, 5)] == [n_labels, int((~ok).sum()), int((shapes.touches_border & ok).sum()),
                                                   int((shapes.euler[ok] != 1).sum())]
    upper = lambda a: float(np.sort(a)[len(a) // 2])
    assert float(line[3]) == pytest.approx(upper(shapes.diameter[ok]), rel=1e-5)
    assert float(line[4]) == pytest.approx(upper(shapes.sphericity[ok]), rel=1e-5)
    return shapes


def test_cli_label_shape_in_a_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([s0, s1, s0]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", "4", "--outer", "2", "--inner", "3", "--silent", "--frames", *paths]

    def run(tag, extra, frames=args):
        r = subprocess.run(frames + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    base = ["--cumulative", "--segment", "otsu:", "--segment-min-voxels", "8", "--label-motion", "rigid", "--contacts"]
    with_shapes = run("s", base + ["--label-shape"])
    plain = run("p", base)
    lines = LINE.findall(with_shapes)
    assert len(lines) == 1 and not LINE.findall(plain)
    keep = lambda text: [l for l in text.splitlines()
                         if l.startswith(("threshold frame", "bodies frame", "displacement frame", "label motion frame", "contacts frame"))]
    assert keep(with_shapes) == keep(plain) and len(keep(plain)) >= 6
    assert with_shapes.index("bodies frame 0") < with_shapes.index("shapes frame 0") < with_shapes.index("label motion frame")
    names = sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("p_"))
    assert sorted(n[2:] for n in os.listdir(tmp_path) if n.startswith("s_")) == sorted(names + ["0_shapes.csv"])
    assert "0_bodies.csv" in names and "0_labels.raw" in names and len(names) > 12
    for name in names:                                                     # every other output byte for byte
        assert open(tmp_path / f"s_{name}", "rb").read() == open(tmp_path / f"p_{name}", "rb").read(), name
    labels = np.fromfile(str(tmp_path / "s_0_labels.raw"), "<i4").reshape(d, h, w)
    n_labels = int(labels.max())
    shapes = check_table(f3d, tmp_path / "s_0_shapes.csv", lines[0], labels, n_labels)
    sizes = [int(r.split(",")[1]) for r in open(tmp_path / "s_0_bodies.csv").read().strip().split("\n")[1:]]
    assert shapes.voxels.tolist() == sizes and n_labels > 3
    # labels from a file, a single pair, nothing else asked for; label 2 is left without a voxel
    labels[labels == 2] = 0
    label_path = str(tmp_path / "labels.raw")
    labels.astype("<i4").tofile(label_path)
    out = run("a", ["--labels", label_path, "--label-shape"], args[:-1])
    lines = LINE.findall(out)
    assert len(lines) == 1 and int(lines[0][1]) == 1
    check_table(f3d, tmp_path / "a_shapes.csv", lines[0], labels, n_labels)
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("a_")) == sorted(["a_shapes.csv"] + [f"a_flow-{c}-{w}-{h}-{d}.raw" for c in "uvw"])
