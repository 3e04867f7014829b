"""The shapes of labelled bodies without a GPU: the numpy restatement (tests/label_shape_ref.py) against a plain loop over the voxels and
against bodies whose sums, Euler number and surface are known; the three direction weights in closed form; the host solve
(f3d_label_shape_solve) against numpy.linalg.eigh of the same covariance and against blocks; the solve under AddressSanitizer and
UBSan in a stand-alone program; the struct layouts; the binding's argument checks; the message of a device library without
f3d_label_shape_sums; and the refusals of bin/flow3d --label-shape.

Bounds of the solve.  Cyclic Jacobi in binary64 is backward stable to a few eps (1.1e-16) of the norm of the matrix, and so is eigh:
eigenvalues are compared to 1e-12 of the trace, which leaves three orders of magnitude.  An eigenvector moves by the perturbation over
the gap to the next eigenvalue, so axes are compared only where the gaps exceed 1e-6 of the trace (then 1e-15 / 1e-6 = 1e-9 in the
direction, far less in |dot|) as |dot| >= 1 - 1e-9.

Measured with the restatement: the ball r <= 20.3 in 48^3 has surface 5156.5 against 4 pi r^2 = 5178.5 (0.42 % low; asserted within
1 %); the torus R = 14, r = 5.2 has surface 2825.5 against 4 pi^2 R r = 2874.0, where (2/3) * faces gives 2709.3."""
import ctypes as C
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import label_shape_ref as ref
from label_motion_ref import voronoi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
HOST = os.path.join(ROOT, "cuda-flow3d_amd", "host")
F32 = np.float32


def one(volume):
    """the row of sums of label 1 of a volume of zeros and ones"""
    sums, info = ref.label_shape_sums(volume, 1)
    assert info["labelled"] == int(volume.sum()) == int(sums["n"][0]) and info["foreign"] == 0
    return sums[0]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (2, 2, 2), (1, 5, 4), (3, 4, 5), (6, 5, 7)], ids=str)
def test_the_restatement_against_a_loop_over_the_voxels(shape):
    rng = np.random.default_rng(sum(shape))
    labels = rng.integers(-1, 5, shape).astype(np.int32)              # background, foreign on both sides (-1 and 4), three bodies
    labels[rng.random(shape) < 0.05] = np.iinfo(np.int32).min
    fast, info = ref.label_shape_sums(labels, 3)
    slow, info_slow = ref.label_shape_sums_loops(labels, 3)
    assert ref.as_rows(fast) == slow and info == info_slow
    assert sum(info.values()) == np.prod(shape) and int(fast["n"].sum()) == info["labelled"]
    spare, _ = ref.label_shape_sums(labels, 6)                        # labels nobody carries: the empty encoding
    assert (spare["n"][4:] == 0).all() and (spare["lo"][4:] == 0).all() and (spare["hi"][4:] == -1).all()
    assert spare[:3].tobytes() == fast.tobytes()


@pytest.mark.parametrize("a,b,c", [(1, 1, 1), (5, 1, 1), (1, 4, 3), (7, 5, 2), (4, 6, 5)])
def test_a_block_in_closed_form(a, b, c):
    volume = np.zeros((c + 3, b + 2, a + 4), np.int32)
    volume[2:2 + c, 1:1 + b, 3:3 + a] = 1
    s = one(volume)
    assert int(s["n"]) == a * b * c and s["lo"].tolist() == [3, 1, 2] and s["hi"].tolist() == [2 + a, b, 1 + c]
    size = (a, b, c)
    assert s["pairs"].tolist() == [math.prod(size[i] - abs(d[i]) for i in range(3)) for d in ref.DIRECTIONS]
    assert s["squares"].tolist() == [(a - 1) * (b - 1) * c, (a - 1) * b * (c - 1), a * (b - 1) * (c - 1)]
    assert int(s["cubes"]) == (a - 1) * (b - 1) * (c - 1) and s["border"].tolist() == [0, 0, 0]
    assert ref.euler(s) == 1 and ref.faces(s) == 2 * (a * b + a * c + b * c)
    tight = one(np.ones((c, b, a), np.int32))                          # the block is the box: every face voxel is on the border
    assert tight["border"].tolist() == [2 * b * c, 2 * a * c, 2 * a * b] and tight["pairs"].tolist() == s["pairs"].tolist()


def test_euler_numbers_of_a_ball_a_shell_a_torus_and_two_caps():
    ball = ref.ball(20.3)
    assert ref.euler(one(ball)) == 1
    shell = ball.copy()
    shell[ref.ball(8.2) == 1] = 0
    assert ref.euler(one(shell)) == 2                                   # one piece, one cavity
    assert ref.euler(one(ref.torus(14, 5.2))) == 0                      # one piece, one tunnel
    caps = ball.copy()
    caps[23:25] = 0                                                     # the planes z = 23, 24 removed: two pieces under one label
    assert ref.euler(one(caps)) == 2


def test_the_weights_are_the_shares_of_the_sphere():
    shares = ref.sphere_shares()
    assert abs(3 * shares[0] + 6 * shares[1] + 4 * shares[2] - 1.0) < 1e-12
    for given, exact in zip(ref.WEIGHTS, shares):
        assert abs(given - exact) < 1e-9                                # the header gives ten decimals
    text = open(os.path.join(ROOT, "include", "f3d_host.h")).read()
    for given in ref.WEIGHTS:
        assert f"{given:.10f}" in text and f"{given:.10f}" in open(os.path.join(HOST, "label_shape.cpp")).read()


def test_the_surface_estimate_on_a_ball_and_a_torus():
    s = one(ref.ball(20.3))
    exact = 4 * math.pi * 20.3 ** 2
    print("ball: surface", ref.surface(s), "exact", exact, "faces", ref.faces(s))
    assert abs(ref.surface(s) - exact) < 0.01 * exact
    assert ref.faces(s) > 1.4 * exact                                   # the staircase area is no estimate of it
    t = one(ref.torus(14, 5.2))
    exact = 4 * math.pi ** 2 * 14 * 5.2
    print("torus: surface", ref.surface(t), "exact", exact, "2/3 faces", 2 / 3 * ref.faces(t))
    assert abs(ref.surface(t) - exact) < abs(2 / 3 * ref.faces(t) - exact)


# ---- the host solve --------------------------------------------------------------------------------------------------------------------------

def bodies():
    """sums of bodies of many shapes: Voronoi cells, a ball, a torus, a rod off the axes, a plate, single voxels and an empty label"""
    volume = voronoi((20, 24, 28), 12, seed=3)
    z, y, x = np.meshgrid(np.arange(20), np.arange(24), np.arange(28), indexing="ij")
    volume[(x - 17.5) ** 2 + (y - 9.5) ** 2 + (z - 10.5) ** 2 <= 6.4 ** 2] = 13     # a ball
    volume[(np.abs(x - y) <= 1) & (np.abs(z - 0.5 * x - 3) <= 1)] = 14      # a rod along (2, 2, 1)
    volume[5, 2:20, 3:9] = 15                                              # a plate one voxel thick
    volume[0, 0, 0] = 16
    volume[19, 23, 27] = 17
    sums, _ = ref.label_shape_sums(volume, 19)                             # 18 and 19 have no voxel
    return volume, sums


def test_the_solve_against_eigh_of_the_same_covariance(f3d):
    volume, sums = bodies()
    shapes = f3d.solve_label_shapes(sums)
    assert len(shapes) == 19 and shapes.status.tolist() == [ref.OK] * 17 + [ref.EMPTY] * 2
    compared = 0
    for i in range(17):
        row = sums[i]
        cov = ref.covariance(row)
        values, vectors = np.linalg.eigh(cov)
        values, vectors = values[::-1], vectors[:, ::-1]
        trace = float(np.trace(cov))
        got = shapes.semi_axes[i] ** 2 / 5.0
        assert np.all(np.diff(got) <= 0) and np.abs(got - values).max() <= 1e-12 * trace, (i, got, values)
        axes = shapes.axes[i]
        assert np.abs(axes @ axes.T - np.eye(3)).max() < 1e-14              # unit and orthogonal
        for j in range(3):
            big = int(np.argmax(np.abs(axes[j])))
            assert axes[j, big] > 0                                        # the sign rule
            gaps = [abs(values[j] - values[k]) for k in range(3) if k != j]
            if min(gaps) > 1e-6 * trace:
                assert abs(float(axes[j] @ vectors[:, j])) >= 1 - 1e-9, (i, j)
                compared += 1
        n = int(row["n"])
        assert shapes.voxels[i] == n and shapes.box[i].tolist() == [row["lo"].tolist(), row["hi"].tolist()]
        assert shapes.border[i].tolist() == row["border"].tolist()
        assert np.allclose(shapes.centroid[i], [int(v) / n for v in row["s1"]], rtol=1e-15, atol=0)
        assert math.isclose(shapes.diameter[i], (6 * n / math.pi) ** (1 / 3), rel_tol=1e-14)
        assert shapes.faces[i] == ref.faces(row) and shapes.euler[i] == ref.euler(row)
        assert math.isclose(shapes.surface[i], ref.surface(row), rel_tol=1e-14)
        assert math.isclose(shapes.sphericity[i], ref.sphericity(row), rel_tol=1e-14)
    assert compared >= 30                                                  # most axes of these bodies are well separated
    # centroids are those of the voxels
    z, y, x = np.nonzero(volume == 14)
    assert np.allclose(shapes.centroid[13], [x.mean(), y.mean(), z.mean()], rtol=1e-13)
    rod = shapes.axes[13, 0]
    assert abs(rod @ np.array([2, 2, 1]) / 3) > 0.99                       # the long axis of the rod
    assert abs(shapes.axes[14, 2] @ np.array([0, 0, 1.0])) == 1.0          # the short axis of the plate
    assert shapes.touches_border.tolist() == [bool(r["border"].sum()) for r in sums]
    assert shapes.touches_border[15] and shapes.touches_border[16] and not shapes.touches_border[14]


def test_the_solve_of_an_empty_label_and_of_blocks(f3d):
    a, b, c = 9, 4, 6
    volume = np.zeros((c + 2, b + 2, a + 2), np.int32)
    volume[1:1 + c, 1:1 + b, 1:1 + a] = 2
    sums, _ = ref.label_shape_sums(volume, 3)
    shapes = f3d.solve_label_shapes(sums)
    assert shapes.status.tolist() == [ref.EMPTY, ref.OK, ref.EMPTY]
    for i in (0, 2):
        assert shapes.voxels[i] == 0 and shapes.box[i].tolist() == [[0, 0, 0], [-1, -1, -1]] and shapes.faces[i] == 0 and shapes.euler[i] == 0
        for name in ("centroid", "diameter", "semi_axes", "axes", "surface", "sphericity"):
            assert np.isnan(getattr(shapes, name)[i]).all(), name
        assert not shapes.touches_border[i]
    assert np.allclose(shapes.semi_axes[1], [math.sqrt(5 * k * k / 12) for k in (a, c, b)], rtol=1e-14)    # descending: 9, 6, 4
    assert shapes.axes[1].tolist() == [[1, 0, 0], [0, 0, 1], [0, 1, 0]]
    assert shapes.centroid[1].tolist() == [1 + (a - 1) / 2, 1 + (b - 1) / 2, 1 + (c - 1) / 2]
    assert shapes.euler[1] == 1 and shapes.faces[1] == 2 * (a * b + a * c + b * c) and shapes.sphericity[1] < 1
    table = shapes.as_table()
    assert table[1]["label"] == 2 and table[1]["status"] == "ok" and table[0]["status"] == "empty" and table[1]["voxels"] == a * b * c
    assert table[1]["box"] == [[1, 1, 1], [a, b, c]] and table[1]["touches_border"] is False and table[1]["euler"] == 1
    assert set(table[1]) == {"label", "status", "voxels", "box", "border", "touches_border", "centroid", "diameter", "semi_axes", "axes",
                             "faces", "surface", "sphericity", "euler"}
    ball = f3d.solve_label_shapes(ref.label_shape_sums(ref.ball(20.3), 1)[0])
    assert abs(ball.sphericity[0] - 1) < 0.01 and abs(ball.diameter[0] - 40.6) < 0.1
    assert np.allclose(ball.semi_axes[0], 20.3, rtol=0.005)
    assert len(f3d.solve_label_shapes(sums[:0])) == 0


def test_the_solve_under_the_sanitizers(tmp_path):
    """host/label_shape.cpp and tests/label_shape_solve_main.cpp built into a program of their own with AddressSanitizer and UBSan"""
    exe = tmp_path / "label_shape_solve"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(HOST, "label_shape.cpp"), os.path.join(ROOT, "tests", "label_shape_solve_main.cpp"), "-o", str(exe)],
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
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(struct f3d_label_shape_sums), offsetof(struct f3d_label_shape_sums, lo),
                 offsetof(struct f3d_label_shape_sums, hi), offsetof(struct f3d_label_shape_sums, s1), offsetof(struct f3d_label_shape_sums, s2),
                 offsetof(struct f3d_label_shape_sums, pairs), offsetof(struct f3d_label_shape_sums, squares),
                 offsetof(struct f3d_label_shape_sums, cubes), offsetof(struct f3d_label_shape_sums, border));
          printf("%zu %zu\\n", sizeof(f3d_label_shape_info), offsetof(f3d_label_shape_info, labelled));
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(f3d_label_shape), offsetof(f3d_label_shape, voxels),
                 offsetof(f3d_label_shape, box_lo), offsetof(f3d_label_shape, box_hi), offsetof(f3d_label_shape, border),
                 offsetof(f3d_label_shape, centroid), offsetof(f3d_label_shape, diameter), offsetof(f3d_label_shape, semi_axes),
                 offsetof(f3d_label_shape, axes), offsetof(f3d_label_shape, faces), offsetof(f3d_label_shape, surface),
                 offsetof(f3d_label_shape, sphericity), offsetof(f3d_label_shape, euler));
          printf("%d %d\\n", F3D_LABEL_OK, F3D_LABEL_EMPTY);
          return 0;
        }'''))
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    S, I, T = f3d.LabelShapeSums, f3d.LabelShapeInfo, f3d.LabelShape
    assert ([int(x) for x in lines[0].split()]
            == [C.sizeof(S), S.lo.offset, S.hi.offset, S.s1.offset, S.s2.offset, S.pairs.offset, S.squares.offset, S.cubes.offset, S.border.offset]
            == [288, 8, 32, 56, 80, 128, 232, 256, 264])
    assert [int(x) for x in lines[1].split()] == [C.sizeof(I), I.labelled.offset] == [24, 16]
    fields = ("voxels", "box_lo", "box_hi", "border", "centroid", "diameter", "semi_axes", "axes", "faces", "surface", "sphericity", "euler")
    assert ([int(x) for x in lines[2].split()] == [C.sizeof(T)] + [getattr(T, n).offset for n in fields]
            == [248, 8, 16, 40, 64, 88, 112, 120, 144, 216, 224, 232, 240])
    assert [int(x) for x in lines[3].split()] == [ref.OK, ref.EMPTY] == [f3d.LABEL_STATUS.index("ok"), f3d.LABEL_STATUS.index("empty")]
    assert f3d._SHAPE_SUMS_DTYPE == ref.SUMS_DTYPE and f3d._SHAPE_SUMS_DTYPE.itemsize == 288 and f3d._SHAPE_DTYPE.itemsize == 248
    for name in fields:
        assert f3d._SHAPE_DTYPE.fields[name][1] == getattr(T, name).offset, name
    for name in ref.SUMS_DTYPE.names:
        assert ref.SUMS_DTYPE.fields[name][1] == getattr(S, name).offset, name


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_label_shape_sums"]),
                                              ("f3d_host.h", "host", ["f3d_label_shape_solve", "f3d_flow_label_shapes_compute"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    text = open(os.path.join(ROOT, "include", header)).read()
    if header == "f3d.h":                                      # the definition stands in the header in full
        for needle in ("(1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1) (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1)",
                       "lo[i] = 0 and hi[i] = -1", "xx yy zz xy xz yz", "a voxel of a box one voxel thick along i counts twice",
                       "container padding is never read", "s2 < 2^61", "2^31 - 1 in the box", "n_labels outside 1 .. 2^22",
                       "288 B per label"):
            assert needle in text, needle
    else:
        for needle in ("m_ik = n s2_ik - s1_i s1_k exactly in a 128-bit integer", "12 sweeps over the pairs (0,1) (0,2)", "sqrt(5.0 * l_i)",
                       "cbrt(6.0 * N / pi)", "cbrt(pi * ((6.0 * N) * (6.0 * N))) / surface", "pieces - tunnels + cavities",
                       "component of largest magnitude is positive"):
            assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    fn = f3d._label_shape_entry()
    assert len(fn.argtypes) == 7
    good = np.ones((3, 4, 5), np.int64)
    with pytest.raises(ValueError, match="integers"):
        f3d.label_shape_sums(np.zeros((3, 4, 5), F32))
    with pytest.raises(ValueError, match="integers"):
        f3d.label_shapes(good[0])
    with pytest.raises(ValueError, match="int32"):
        f3d.label_shape_sums(good * 2 ** 31)
    with pytest.raises(ValueError, match="n_labels"):
        f3d.label_shape_sums(good * 0)
    with pytest.raises(ValueError, match="n_labels"):
        f3d.label_shapes(good, n_labels=(1 << 22) + 1)
    with pytest.raises(ValueError, match="non-empty"):
        f3d.label_shape_sums(np.ones((0, 4, 5), np.int32), n_labels=1)
    with pytest.raises(ValueError, match="one-dimensional"):
        f3d.solve_label_shapes(np.zeros((2, 2), ref.SUMS_DTYPE))
    host = f3d.host()
    rows, out = (f3d.LabelShapeSums * 1)(), (f3d.LabelShape * 1)()
    for args in ((None, 1, out), (rows, 1, None)):
        assert host.f3d_label_shape_solve(*args) != 0 and b"f3d_label_shape_solve" in host.f3d_host_last_error()
    assert host.f3d_flow_label_shapes_compute(None, None, 1, out, None) != 0
    assert b"f3d_flow_label_shapes_compute" in host.f3d_host_last_error()
    assert hasattr(f3d.OpticalFlow, "label_shapes")


CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    labels = np.ones((D, H, W), np.int32); labels[:, :, 10:] = 2
    for call in (lambda: flow.label_shapes(labels), lambda: pkg.label_shape_sums(labels), lambda: pkg.label_shapes(labels)):
        try:
            call(); raise SystemExit("a call succeeded without f3d_label_shape_sums")
        except pkg.F3dError as e:
            assert "f3d_label_shape_sums" in str(e), str(e)
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_label_shape_sums: libf3d_host.so built against it must still load (RTLD_NOW), and the shape
    calls must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_label_shape_sums" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("case,needle", [("no-labels", "--label-shape needs --labels FILE or --segment"),
                                         ("partial", "--label-shape needs the resident"), ("concurrent", "--label-shape needs the resident"),
                                         ("segment-partial", "the resident"), ("missing-file", "cannot read"), ("no-body", "largest label")])
def test_flow3d_label_shape_argument_errors(tmp_path, case, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(2):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))

    def label_file(name, values):
        p = tmp_path / name
        np.asarray(values, np.int32).tofile(p)
        return str(p)

    good = label_file("labels.raw", np.ones(64))
    extra = {"no-labels": ["--label-shape"],
             "partial": ["--labels", good, "--label-shape", "--partial"],
             "concurrent": ["--labels", good, "--label-shape", "--concurrent", "2"],
             "segment-partial": ["--segment", "0.5:", "--label-shape", "--partial"],
             "missing-file": ["--labels", str(tmp_path / "nothing.raw"), "--label-shape"],
             "no-body": ["--labels", label_file("zero.raw", np.zeros(64)), "--label-shape"]}[case]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "[(--labels FILE | --segment ...) --label-shape]" in run.stdout
    assert "[--labels FILE --contacts [--contact-min-faces K]]" in run.stdout                       # the earlier usage text is all there
    assert "3D optical flow" not in run.stdout                                                   # before any device is touched
    assert not any("shapes" in n or "flow-" in n for n in os.listdir(tmp_path))
