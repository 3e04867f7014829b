"""The connected bodies of a thresholded volume without a GPU: the restatement (tests/components_ref.py) against scipy.ndimage.label
renumbered by first raster occurrence and against a flood fill, the closed forms the large GPU case relies on, the union-find of the
kernels (csrc/f3d_union_find.h) run by several host threads under AddressSanitizer and UBSan in a stand-alone program, the struct
layout, the binding's argument checks, the message of a device library without f3d_label_components, and the refusals of
bin/flow3d --segment."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import components_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (2, 2, 3), (33, 5, 65), (70, 9, 130)]      # [d, h, w]: those of the GPU tests
ids = lambda s: "x".join(map(str, s[::-1])) if isinstance(s, tuple) else str(s)


def by_first_occurrence(found):
    """scipy's labels renumbered in the order in which they first occur in a raster scan (its own order is not relied upon)"""
    flat = found.ravel()
    values, first = np.unique(flat[flat > 0], return_index=True)
    order = np.zeros(int(flat.max()) + 1, np.int64)
    order[values[np.argsort(first)]] = np.arange(1, len(values) + 1)
    return order[found]


def scipy_components(mask, min_voxels):
    """(labels, sizes) of the definition in include/f3d.h, built on scipy.ndimage.label with its default six-neighbour structure"""
    from scipy import ndimage
    found, count = ndimage.label(mask)
    assert ndimage.generate_binary_structure(3, 1).sum() == 7
    comp = by_first_occurrence(found)
    sizes = np.bincount(comp.ravel(), minlength=count + 1)[1:]
    kept = sizes >= min_voxels
    number = np.concatenate([[0], np.where(kept, np.cumsum(kept), 0)])
    return number[comp].astype(np.int32), sizes[kept].astype(np.uint64), sizes


@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_restatement_against_scipy(shape, layout):
    mask = ref.layout_mask(layout, shape)
    volume = ref.as_volume(mask, 0.75, 0.25)
    for min_voxels in (1, 2, 27):
        labels, sizes, info = ref.label_components(volume, 0.5, 1.0, min_voxels)
        want, want_sizes, all_sizes = scipy_components(mask, min_voxels)
        assert np.array_equal(labels, want) and np.array_equal(sizes, want_sizes)
        assert info == dict(foreground=int(mask.sum()), background=int((~mask).sum()), nan=0, n_components=len(all_sizes),
                            n_labels=len(want_sizes), dropped_components=len(all_sizes) - len(want_sizes),
                            dropped_voxels=int(all_sizes.sum() - want_sizes.sum()), largest=int(all_sizes.max(initial=0)))
    if shape == SHAPES[-1]:                                             # the layouts are what they claim to be
        count = info["n_components"]
        if layout.startswith("serpentine"):
            assert count == 1 and info["largest"] == mask.sum()
        if layout == "checker":
            assert count == mask.sum() == (mask.size + 1) // 2
        if layout == "diagonal":
            assert count == mask.sum() > 100
        if layout == "voronoi":
            assert count >= 20
        if layout.startswith("comb"):
            d, h, w = shape
            arms = {"comb-x": (h + 1) // 2 * ((d + 1) // 2), "comb-y": (w + 1) // 2 * ((d + 1) // 2), "comb-z": (w + 1) // 2 * ((h + 1) // 2)}[layout]
            assert count < arms                                         # arms are joined in pairs, at the far end only
        if layout == "noise-0.31":
            assert count > 1000 and info["largest"] > 100


@pytest.mark.parametrize("seed", range(12))
def test_the_restatement_against_a_flood_fill(seed):
    rng = np.random.default_rng(seed)
    shape = tuple(int(k) for k in rng.integers(1, [5, 6, 7]))          # at most 4 x 5 x 6 [d, h, w]
    volume = rng.random(shape).astype(F32)
    volume[rng.random(shape) < 0.1] = np.nan
    lo, hi = (0.2, 0.8) if seed % 2 else (-np.inf, 0.55)
    for min_voxels in (1, 2, 3):
        labels, sizes, info = ref.label_components(volume, lo, hi, min_voxels)
        want, want_sizes = ref.flood_fill(ref.foreground(volume, lo, hi), min_voxels)
        assert np.array_equal(labels, want) and np.array_equal(sizes, want_sizes)
        assert info["nan"] == np.isnan(volume).sum() and info["foreground"] + info["background"] == volume.size
        assert info["foreground"] - info["dropped_voxels"] == (labels > 0).sum() == sizes.sum()


def test_the_closed_forms_of_the_large_case():
    shape, brick = (9, 11, 23), (4, 3, 5)
    mask, labels, sizes = ref.bricks(shape, brick)
    got, got_sizes, info = ref.label_components(ref.as_volume(mask), 0.5, np.inf, 1)
    assert np.array_equal(got, labels) and np.array_equal(got_sizes, sizes) and info["n_labels"] == 3 * 4 * 5
    mask = ref.checkerboard(shape)
    got, got_sizes, info = ref.label_components(ref.as_volume(mask), 0.5, np.inf, 1)
    assert np.array_equal(got, np.where(mask, np.cumsum(mask.ravel()).reshape(shape), 0)) and (got_sizes == 1).all()


def test_the_values_the_definition_names():
    v = np.array([[[0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, 2.0, np.nextafter(F32(2), F32(3))]]], F32)
    mask = lambda lo, hi: ref.foreground(v, lo, hi)[0, 0].tolist()
    assert mask(0.0, 2.0) == [True, True, False, False, False, True, False, True, True, False]       # -0.0 == 0.0; lo and hi themselves
    assert mask(-np.inf, np.inf) == [True, True, False, True, True, True, True, True, True, True]    # only the NaN is left out
    assert mask(1e-45, 1e-45) == [False, False, False, False, False, True, False, False, False, False]   # a denormal compares as its value
    assert mask(-np.inf, -1e-45) == [False, False, False, False, True, False, True, False, False, False]


# ---- the union-find of the kernels on the host, under sanitizers --------------------------------------------------------------------

def test_the_union_find_header_with_host_threads_under_sanitizers(tmp_path):
    """csrc/f3d_union_find.h with std::atomic behind its primitives (tests/components_uf_main.cpp, a program of its own): the three
    passes with 1, 2 and 7 threads on the serpentine and the noise layouts against a sequential flood fill, built with
    -fsanitize=address,undefined and run here on the CPU"""
    exe = tmp_path / "components_uf"
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-pthread", "-I", os.path.join(ROOT, "cuda-flow3d_amd", "csrc"), os.path.join(ROOT, "tests", "components_uf_main.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok union-find"), (run.stdout[-2000:], run.stderr[-3000:])
    assert run.stdout.count(" 0 wrong") == 15 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# ---- packaging ---------------------------------------------------------------------------------------------------------------------------

def test_struct_layout_against_the_header(f3d, tmp_path):
    src = tmp_path / "sizes.c"
    names = ref.INFO
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "f3d_host.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(f3d_component_info));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(f3d_component_info, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = f3d.ComponentInfo
    assert [n for n, _ in T._fields_] == list(names)
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names] == [64] + [8 * i for i in range(8)]


@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_label_components"]),
                                              ("f3d_host.h", "host", ["f3d_flow_labels_compute", "f3d_flow_labels_end",
                                                                      "f3d_flow_labels_download"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    if header == "f3d.h":                                          # the definition stands in the header in full
        text = open(os.path.join(ROOT, "include", header)).read()
        for needle in ("lo <= s && s <= hi", "x + W (y + H z)", "smallest linear box index", "ascending order of root",
                       "2^31 - 1", "sizes given with capacity 0", "no float instruction touches a label"):
            assert needle in text, needle


def test_the_binding_checks_its_arguments(f3d):
    fn = f3d._components_entry()
    assert len(fn.argtypes) == 11
    good = np.zeros((3, 4, 5), F32)
    for kw in (dict(lo=np.nan), dict(hi=np.nan), dict(lo=2.0, hi=1.0), dict(lo=np.inf, hi=-np.inf)):
        with pytest.raises(ValueError, match="lo and hi"):
            f3d.label_components(good, **kw)
    for k in (0, -3):
        with pytest.raises(ValueError, match="min_voxels"):
            f3d.label_components(good, min_voxels=k)
    for bad in (np.zeros((4, 5), F32), np.zeros((0, 4, 5), F32)):
        with pytest.raises(ValueError, match="volume"):
            f3d.label_components(bad)
    host = f3d.host()
    info = f3d.ComponentInfo()
    sizes, count = C.POINTER(C.c_ulonglong)(), C.c_size_t(0)
    assert host.f3d_flow_labels_compute(None, 0, 0.0, 1.0, 1, C.byref(sizes), C.byref(count), C.byref(info)) != 0
    assert b"f3d_flow_labels_compute" in host.f3d_host_last_error()
    assert host.f3d_flow_labels_end(None) != 0 and b"f3d_flow_labels_end" in host.f3d_host_last_error()
    assert host.f3d_flow_labels_download(None, None) != 0 and b"f3d_flow_labels_download" in host.f3d_host_last_error()
    assert hasattr(f3d.OpticalFlow, "segment") and hasattr(f3d.OpticalFlow, "segment_end")
    c = f3d.Components(np.zeros((1, 1, 2), np.int32), np.zeros(0, np.uint64), dict.fromkeys(ref.INFO, 0))
    assert c.n_labels == 0 and len(c) == 0


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
    for call in (lambda: flow.segment(0.4), lambda: pkg.label_components(f0, 0.4)):
        try:
            call(); raise SystemExit("a call succeeded without f3d_label_components")
        except pkg.F3dError as e:
            assert "f3d_label_components" in str(e), str(e)
    flow.segment_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_label_components: libf3d_host.so built against it must still load (RTLD_NOW) and solve
    flows, and ComputeLabels must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_label_components" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("case,needle", [("with-labels", "--segment takes the place of --labels"),
                                         ("min-only", "--segment-min-voxels needs --segment"), ("no-colon", "usage"), ("two-colons", "usage"),
                                         ("not-a-number", "usage"), ("trailing", "usage"), ("nan", "usage"), ("lo-above-hi", "LO is above HI"),
                                         ("zero-min", "usage"), ("bad-min", "usage"), ("missing-value", "usage"),
                                         ("partial", "--segment needs the resident"), ("concurrent", "--segment needs the resident"),
                                         ("contacts-sequence", "--cumulative")])
def test_flow3d_segment_argument_errors(tmp_path, case, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    good = tmp_path / "labels.raw"
    np.ones(64, np.int32).tofile(good)
    frames = paths if case == "contacts-sequence" else paths[:2]
    extra = {"with-labels": ["--segment", "0.4:", "--labels", str(good), "--contacts"],
             "min-only": ["--segment-min-voxels", "5"],
             "no-colon": ["--segment", "0.4"], "two-colons": ["--segment", "0.1:0.2:0.3"], "not-a-number": ["--segment", "low:"],
             "trailing": ["--segment", "0.4x:"], "nan": ["--segment", "nan:"], "lo-above-hi": ["--segment", "0.5:0.25"],
             "zero-min": ["--segment", "0.4:", "--segment-min-voxels", "0"], "bad-min": ["--segment", "0.4:", "--segment-min-voxels", "few"],
             "missing-value": ["--segment"],
             "partial": ["--segment", "0.4:", "--partial"], "concurrent": ["--segment", ":0.4", "--concurrent", "2"],
             "contacts-sequence": ["--segment", "0.4:", "--contacts"]}[case]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *frames, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--segment LO:HI [--segment-min-voxels K]]" in run.stdout
    assert "[--labels FILE --contacts [--contact-min-faces K]]" in run.stdout                    # the earlier usage text is all there
    assert "3D optical flow" not in run.stdout                                                   # before any device is touched
    assert not any("labels" in n and n != "labels.raw" or "bodies" in n or "flow-" in n for n in os.listdir(tmp_path))
