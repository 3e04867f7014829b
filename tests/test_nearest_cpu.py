"""The exact nearest-seed transform and the split of touching bodies without a GPU: the separable restatement (tests/nearest_ref.py)
against the brute-force definition and against scipy.ndimage.distance_transform_edt, the split restatement's identity at core_d2 = 1 and
its result on the sphere packing, the line routine of the kernels (csrc/f3d_envelope.h) in a stand-alone program under AddressSanitizer
and UBSan, the struct layouts, the bindings' argument checks, the messages of a device library without the two entries, and the
refusals of bin/flow3d --segment-split."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import components_ref as cref
import contacts_ref
import nearest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SMALL = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (2, 3, 4), (11, 5, 9), (5, 9, 7)]                      # [d, h, w], up to 9 x 5 x 11
ids = lambda s: "x".join(map(str, s[::-1])) if isinstance(s, tuple) else str(s)


@pytest.mark.parametrize("mode", ["nonzero", "zero"])
@pytest.mark.parametrize("density", [0, 0.02, 0.1, 0.5, 1])
@pytest.mark.parametrize("shape", SMALL, ids=ids)
def test_the_separable_form_with_the_tie_rule_is_the_brute_force_minimum(shape, density, mode):
    rng = np.random.default_rng(3)
    for _ in range(3):
        values = ((rng.random(shape) < density) * rng.integers(1, 9, shape)).astype(np.int32)
        a, b = ref.nearest_brute(values, mode), ref.nearest_separable(values, mode)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        seeds = ref.seed_mask(values, mode)
        if seeds.any():
            assert (a[0][seeds] == 0).all() and np.array_equal(np.flatnonzero(seeds), a[1][seeds])     # a seed is its own nearest seed
            assert a[3]["unreached"] == 0
        else:
            assert (a[0] == 2 ** 31 - 1).all() and (a[1] == -1).all() and not a[2].any() and a[3]["unreached"] == values.size


@pytest.mark.parametrize("layout", ["checker", "pair-x", "pair-diagonal", "face-z1", "noise-0.001", "noise-0.3"])
def test_the_layouts_of_the_gpu_tests_on_a_small_box_against_brute_force(layout):
    values = ref.layout_mask(layout, (7, 5, 9)).astype(np.int32) * 4
    a, b = ref.nearest_brute(values), ref.nearest_separable(values)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("density", [0.001, 0.05, 0.6])
def test_d2_is_scipys_euclidean_distance_squared(density):
    from scipy import ndimage
    mask = ~cref.noise((33, 20, 65), density, seed=9)                    # scipy: distance of the non-zero voxels to the nearest zero
    assert not mask.all()
    edt = ndimage.distance_transform_edt(mask)
    got = ref.distance_squared(mask)
    assert np.array_equal(got, np.rint(edt * edt).astype(np.int64)) and got.dtype == np.int32
    assert np.array_equal(ref.nearest_separable((~mask).astype(np.int32), "nonzero")[0], got)


@pytest.mark.parametrize("layout", cref.LAYOUTS)
def test_the_split_at_core_d2_of_one_is_the_component_labels(layout):
    volume = cref.as_volume(cref.layout_mask(layout, (12, 5, 20)))
    for min_voxels in (1, 3):
        want = cref.label_components(volume, 0.5, 1.0, min_voxels)
        got = ref.split_components(volume, 0.5, 1.0, 1, min_voxels)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == np.uint64
        assert {k: got[2][k] for k in cref.INFO} == want[2]
        assert got[2]["remainder_voxels"] == 0 and got[2]["core_voxels"] == want[2]["foreground"]


def test_the_sphere_packing_splits_into_its_eighteen_spheres():
    mask, count = ref.sphere_packing()
    assert count == 18 and mask.shape == (40, 48, 56)
    volume = cref.as_volume(mask)
    assert cref.label_components(volume, 0.5, 1.0, 1)[2]["n_components"] == 1          # ONE component before the split
    labels, sizes, info = ref.split_components(volume, 0.5, 1.0, 49, 1)
    assert info["n_labels"] == 18 and info["n_cores"] == 18 and info["remainder_voxels"] == 0 and info["remainder_bodies"] == 0
    assert info["connected_components"] == 1 and sizes.min() > 2600 and sizes.sum() == mask.sum()
    contacts, _ = contacts_ref.label_contacts(None, None, None, labels, 18)
    assert len(contacts) >= 31


def test_a_class_of_the_split_need_not_be_connected_and_a_coreless_body_keeps_a_label():
    mask, small = ref.necked_balls()
    labels, sizes, info = ref.split_components(cref.as_volume(mask), 0.5, 1.0, 16, 1)
    assert info["n_labels"] == 3 and info["remainder_bodies"] == 1 and (labels[small] == 3).all() and sizes[2] == small.sum()


# ---- the line routine of the kernels on the host, under sanitizers --------------------------------------------------------------------

def test_the_envelope_header_on_the_host_under_sanitizers(tmp_path):
    """csrc/f3d_envelope.h over plain vectors (tests/nearest_line_main.cpp, a program of its own) against the brute-force line minimum:
    all seeds, none, one at either end, alternating, exact ties at every separator, rising, falling, random; lengths 1, 2, 63, 64, 65,
    300; and the separator against 64-bit floor division.  Built with -fsanitize=address,undefined and run here on the CPU"""
    exe = tmp_path / "nearest_line"
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cuda-flow3d_amd", "csrc"), os.path.join(ROOT, "tests", "nearest_line_main.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok envelope"), (run.stdout[-2000:], run.stderr[-3000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 6 * 34 + 2 and all(l.endswith(" 0 wrong") for l in lines[:-1])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("struct,cls,names", [("f3d_nearest_info", "NearestInfo", ref.INFO), ("f3d_split_info", "SplitInfo", ref.SPLIT_INFO)])
def test_struct_layout_against_the_header(f3d, tmp_path, struct, cls, names):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "f3d_host.h"\nint main(void) {\n'
                   f'  printf("%zu\\n", sizeof({struct}));\n' +
                   "".join(f'  printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = getattr(f3d, cls)
    assert [n for n, _ in T._fields_] == list(names)
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names] == [8 * len(names)] + [8 * i for i in range(len(names))]


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_nearest_seed", "f3d_split_components"]),
                                              ("f3d_host.h", "host", ["f3d_flow_labels_split"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    if header == "f3d.h":                                          # the definitions stand in the header in full
        text = open(os.path.join(ROOT, "include", header)).read()
        for needle in ("(squared distance, box index) lexicographically", "smallest box index wins", "F3D_SEED_ZERO", "monotone",
                       "W^2 + H^2 + D^2 <= 2^31 - 1", "No float instruction touches a distance", "12 B per voxel", "32 B per voxel",
                       "equal f3d_label_components' byte for byte", "Euclidean, not geodesic", "remainder of its component"):
            assert needle in text, needle


def test_the_bindings_check_their_arguments(f3d):
    assert len(f3d._nearest_entry().argtypes) == 10 and len(f3d._split_entry().argtypes) == 12
    good = np.zeros((3, 4, 5), np.int32)
    with pytest.raises(ValueError, match="mode"):
        f3d.nearest_seed(good, mode="both")
    for outputs in ((), ("d2", "d2"), ("depth",), "depth"):
        with pytest.raises(ValueError, match="outputs"):
            f3d.nearest_seed(good, outputs=outputs)
    for bad in (np.zeros((4, 5), np.int32), np.zeros((0, 4, 5), np.int32), np.zeros((3, 4, 5), F32), np.full((1, 1, 2), 2 ** 31, np.int64)):
        with pytest.raises(ValueError, match="labels"):
            f3d.nearest_seed(bad)
    with pytest.raises(ValueError, match="mask"):
        f3d.distance_transform(np.zeros((4, 5), bool))
    volume = np.zeros((3, 4, 5), F32)
    for kw in (dict(), dict(radius=2, core_d2=4)):
        with pytest.raises(ValueError, match="exactly one"):
            f3d.split_components(volume, **kw)
    for radius in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            f3d.split_components(volume, radius=radius)
    for core_d2 in (0, -4, 2.5):
        with pytest.raises(ValueError, match="core_d2"):
            f3d.split_components(volume, core_d2=core_d2)
    assert f3d._core_d2(6.5, None) == 43 and f3d._core_d2(7, None) == 49 and f3d._core_d2(None, 49) == 49
    with pytest.raises(ValueError, match="min_voxels"):
        f3d.split_components(volume, core_d2=4, min_voxels=0)
    with pytest.raises(ValueError, match="lo and hi"):
        f3d.split_components(volume, 2.0, 1.0, core_d2=4)
    host = f3d.host()
    info = f3d.SplitInfo()
    sizes, count = C.POINTER(C.c_ulonglong)(), C.c_size_t(0)
    assert host.f3d_flow_labels_split(None, 0, 0.0, 1.0, 4, 1, C.byref(sizes), C.byref(count), C.byref(info)) != 0
    assert b"f3d_flow_labels_split" in host.f3d_host_last_error()
    import inspect
    assert inspect.signature(f3d.OpticalFlow.segment).parameters["split"].default is None


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
    for call, name in ((lambda: flow.segment(0.4, split=4), "f3d_split_components"),
                       (lambda: pkg.split_components(f0, 0.4, core_d2=4), "f3d_split_components"),
                       (lambda: pkg.nearest_seed(f0 > 0.4), "f3d_nearest_seed"),
                       (lambda: pkg.distance_transform(f0 > 0.4), "f3d_nearest_seed")):
        try:
            call(); raise SystemExit("a call succeeded without " + name)
        except pkg.F3dError as e:
            assert name in str(e), str(e)
    flow.segment_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entries():
    """tests/cpu_device defines neither f3d_nearest_seed nor f3d_split_components: libf3d_host.so built against it must still load
    (RTLD_NOW) and solve flows, and the calls must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_nearest_seed" not in names and "f3d_split_components" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- the command line ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["without-segment", "d2-without-segment", "both", "zero-radius", "negative-radius", "inf-radius", "nan-radius",
                                  "bad-radius", "zero-d2", "negative-d2", "bad-d2", "missing-value", "with-labels"])
def test_flow3d_segment_split_argument_errors(tmp_path, case):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(2):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    good = tmp_path / "labels.raw"
    np.ones(64, np.int32).tofile(good)
    seg = ["--segment", "0.4:"]
    extra = {"without-segment": ["--segment-split", "3"], "d2-without-segment": ["--segment-split-d2", "9"],
             "both": seg + ["--segment-split", "3", "--segment-split-d2", "9"], "zero-radius": seg + ["--segment-split", "0"],
             "negative-radius": seg + ["--segment-split", "-2"], "inf-radius": seg + ["--segment-split", "inf"],
             "nan-radius": seg + ["--segment-split", "nan"], "bad-radius": seg + ["--segment-split", "3x"],
             "zero-d2": seg + ["--segment-split-d2", "0"], "negative-d2": seg + ["--segment-split-d2", "-9"],
             "bad-d2": seg + ["--segment-split-d2", "9.5"], "missing-value": seg + ["--segment-split"],
             "with-labels": ["--labels", str(good), "--label-motion", "rigid", "--segment-split", "3"]}[case]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert "usage" in run.stdout and "[--segment-split R | --segment-split-d2 N]" in run.stdout
    assert "[--segment LO:HI [--segment-min-voxels K]]" in run.stdout    # the earlier usage text is all there
    assert "3D optical flow" not in run.stdout                           # before any device is touched
    assert not any("labels" in n and n != "labels.raw" or "bodies" in n or "flow-" in n for n in os.listdir(tmp_path))
