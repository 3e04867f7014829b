"""Solves that start from a given displacement, without a GPU.

 * the Python pyramid of tests/warm_start_ref.py without an initial flow, and with one of zeros, is oracle.compute_flow bit for bit;
 * the quality case: at 14 of 41 levels a guess that is one voxel off per axis ends well below the cold solve and below itself --
   properties of the algorithm on the oracle, not tolerances of the product;
 * the numpy restatement of f3d_initial_flow against a loop over the voxels, the layout of f3d_initial_info against the header;
 * the weak link: against the plain host-memory stand-in (tests/cpu_device, which has no f3d_initial_flow) the host library loads and
   the new calls fail naming the entry;
 * the product's driver on the stand-in of tests/cpu_device_initial, which has the entry: the cases of tests/warm_start_cases.py, in a
   child interpreter pointed at that library directory (see tests/test_host_on_cpu_backend.py for the manner);
 * the stand-alone program tests/initial_flow_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer;
 * the refusals of the command-line tool, each with exit 64 before any device is touched."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import warm_start_ref as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")


def bit_same(a, b):
    return a.shape == b.shape and bool(np.all(np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)))


@pytest.mark.parametrize("shape,shift,kw", [
    (ws.PAIR_SHAPE, ws.PAIR_SHIFT, dict(warp_levels_count=6, outer_iterations_count=5)),
    ((20, 36, 40), (2.0, -1.5, 0.5), dict(gaussian_sigma=0, median_radius=3, warp_levels_count=3))], ids=["24x40x48", "20x36x40"])
def test_the_pyramid_is_the_oracle_without_an_initial_flow_and_with_zeros(oracle, shape, shift, kw):
    f0, f1 = ws.test_pair(shape, shift)
    expected, _ = oracle.compute_flow(f0, f1, **kw)
    assert all(bit_same(g, e) for g, e in zip(ws.pyramid(f0, f1, **kw), expected))
    zeros = ws.constant_flow(shape, (0, 0, 0))
    assert all(bit_same(g, e) for g, e in zip(ws.pyramid(f0, f1, initial=zeros, **kw), expected))


def test_a_guess_one_voxel_off_ends_far_below_the_cold_solve_at_fourteen_levels(oracle):
    """Measured on the oracle: cold 3.30, from the guess 0.505 (ratio 0.15), the guess itself 1.732 (ratio 0.29)."""
    f0, f1 = ws.test_pair()
    guess = ws.constant_flow(f0.shape, ws.PAIR_GUESS)
    cold = ws.rms_error(ws.pyramid(f0, f1, warp_levels_count=14))
    warm = ws.rms_error(ws.pyramid(f0, f1, initial=guess, warp_levels_count=14))
    of_guess = ws.rms_error(guess)
    print(f"rms error against {ws.PAIR_SHIFT}: cold {cold:.4f}, from the guess {warm:.4f}, the guess {of_guess:.4f}")
    assert abs(of_guess - np.sqrt(3.0)) < 1e-6
    assert warm < 0.25 * cold
    assert warm < 0.5 * of_guess


def test_the_restatement_of_the_kernel_against_a_loop_over_the_voxels():
    rng = np.random.default_rng(7)
    for dims in ((1, 1, 1), (7, 5, 3), (9, 4, 2)):
        w, h, d = dims
        for layout in range(4):
            u, v, ww = (rng.uniform(-4, 4, size=(d, h, w)).astype(np.float32) for _ in range(3))
            if layout == 1:
                u[0, 0, 0], ww[-1, -1, -1] = np.nan, np.inf
            if layout == 2:
                u[:], v[:], ww[:] = np.nan, -np.inf, 0.0
            if layout == 3:
                x = np.broadcast_to(np.arange(w, dtype=np.float32), (d, h, w))
                u[:], v[:], ww[:] = np.float32(w - 1) - x, -0.0, 0.0
                u[..., 0] = np.nextafter(np.float32(w - 1), np.float32(np.inf))   # x = 0: one ulp outside
            out, info = ws.initial_flow(u, v, ww)
            loop_out, loop_info = ws.initial_flow_by_loop(u, v, ww)
            assert info == loop_info, (dims, layout, info, loop_info)
            assert all(bit_same(a, b) for a, b in zip(out, loop_out)), (dims, layout)
            if layout == 2:
                assert info["replaced"] == info["voxels"] and info["max_abs"] == 0 and info["leaving"] == 0
            if layout == 3:
                assert info["leaving"] == d * h and info["replaced"] == 0
                assert all(bit_same(a, b) for a, b in zip(out, (u, v, ww))), "a -0 stays -0"


def test_the_layout_of_the_info_matches_the_header(f3d):
    header = open(os.path.join(ROOT, "include", "f3d.h")).read()
    body = re.search(r"typedef struct f3d_initial_info \{(.*?)\} f3d_initial_info;", header, re.S).group(1)
    names = []
    for line in body.split(";"):
        words = line.replace(",", " ").split()
        if words:
            kind = " ".join(w for w in words if w in ("unsigned", "long", "float"))
            names += [(w, kind) for w in words if w not in ("unsigned", "long", "float")]
    assert names == [("voxels", "unsigned long long"), ("replaced", "unsigned long long"), ("leaving", "unsigned long long"), ("max_abs", "float")]
    fields = [(n, {C.c_ulonglong: "unsigned long long", C.c_float: "float"}[t]) for n, t in f3d.InitialInfo._fields_]
    assert fields == names and C.sizeof(f3d.InitialInfo) == 32
    assert [getattr(f3d.InitialInfo, n).offset for n, _ in names] == [0, 8, 16, 24]


def test_argument_checks_of_the_python_entries(f3d):
    a = np.zeros((3, 4, 5), np.float32)
    with pytest.raises(ValueError):
        f3d.initial_flow(a, a, a[1:])
    with pytest.raises(ValueError):
        f3d.initial_flow(a, a, a[0])


WEAK = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in without the entry
    W, H, D = 26, 22, 20
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=3, outer_iterations_count=2)
    guess = tuple(np.zeros((D, H, W), np.float32) for _ in range(3))
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    plain = flow.compute(f0, f1, silent=True, **kw)       # the host library loads and solves without the entry
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    calls = [lambda: pkg.initial_flow(*guess), lambda: flow.set_initial(guess), lambda: flow.set_initial("flow"),
             lambda: flow.compute(f0, f1, silent=True, initial=guess, **kw), lambda: flow.compute_resident(silent=True, initial="flow", **kw),
             lambda: list(flow.compute_sequence([f0, f1], initial=guess, **kw))]
    for call in calls:
        try:
            call(); raise SystemExit("a call succeeded without f3d_initial_flow")
        except pkg.F3dError as e:
            assert "f3d_initial_flow" in str(e), str(e)
    again = flow.compute(f0, f1, silent=True, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    flow.destroy()
    pkg.shutdown()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_entry_and_the_calls_name_it():
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_initial_flow" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", WEAK], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


DRIVER = textwrap.dedent('''
    import importlib, os, sys
    sys.path.insert(0, os.environ["F3D_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["F3D_ROOT"], "tests"))
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in with f3d_initial_flow
    import warm_start_cases as cases
    what = sys.argv[1]
    assert hasattr(pkg.hip(), "f3d_initial_flow")
    if what == "arrays":
        cases.check_from_arrays(pkg, "six_levels")        # initial=None against the oracle's bits pins RunPyramid's null path too
    elif what == "flow":
        cases.check_from_flow(pkg, "six_levels")
    elif what == "trajectory":
        cases.check_from_trajectory(pkg, "six_levels")
    elif what == "holes":
        cases.check_holes(pkg)
    elif what == "levels":
        cases.check_levels_one_and_zero(pkg)
        cases.check_zeros_are_the_plain_call(pkg)
        cases.check_refusals(pkg)
    elif what == "sequences":
        cases.check_sequences(pkg)
    pkg.shutdown()
    print("ok", what)
''')


@pytest.fixture(scope="module")
def with_entry(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpu_device_initial"))
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpu_device_initial"), "OUT=" + out, "all", "main", "-j4"], check=True,
                   stdout=subprocess.DEVNULL)
    return out


@pytest.mark.parametrize("what", ["arrays", "flow", "trajectory", "holes", "levels", "sequences"])
def test_the_driver_on_the_cpu_backend_equals_the_pyramid(with_entry, what):
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=with_entry, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", DRIVER, what], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"ok {what}" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_the_host_memory_entry_at_its_boundaries_under_asan_and_ubsan(with_entry):
    out = subprocess.run([os.path.join(with_entry, "initial_flow_main")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-1500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-3000:]


REFUSALS = {
    "total-cumulative": (3, ["--total", "--cumulative"], "--total solves frame 0 -> frame k+1 directly"),
    "total-warm-start": (3, ["--total", "--warm-start"], "--warm-start belongs to consecutive pairs"),
    "total-partial": (3, ["--total", "--partial"], "--total needs the resident driver"),
    "total-concurrent": (3, ["--total", "--concurrent", "2"], "--total needs the resident driver"),
    "warm-start-partial": (3, ["--warm-start", "--partial"], "--warm-start needs the resident driver"),
    "warm-start-concurrent": (3, ["--warm-start", "--concurrent", "2"], "--warm-start needs the resident driver"),
    "initial-partial": (2, ["--initial-flow", "U", "V", "W", "--partial"], "--initial-flow needs the resident driver"),
    "initial-concurrent": (3, ["--initial-flow", "U", "V", "W", "--concurrent", "2"], "--initial-flow needs the resident driver"),
    "initial-two-files": (2, ["--initial-flow", "U", "V"], "--initial-flow takes three files"),
    "initial-no-file": (2, ["--initial-flow", "--silent"], "--initial-flow takes three files"),
    "initial-four-files": (2, ["--initial-flow", "U", "V", "W", "U"], "--initial-flow takes three files"),
    "initial-wrong-size": (2, ["--initial-flow", "U", "V", "SHORT"], "not a file of 4 x 4 x 4 float32 values"),
    "initial-missing": (2, ["--initial-flow", "U", "V", "NOWHERE"], "not a file of 4 x 4 x 4 float32 values"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_flow3d_refuses_before_any_device_is_touched(tmp_path, case):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    frames, extra, needle = REFUSALS[case]
    paths = []
    for i in range(frames):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    files = {}
    for name in "UVW":
        files[name] = str(tmp_path / f"guess_{name}.raw")
        np.zeros((4, 4, 4), np.float32).tofile(files[name])
    files["SHORT"] = str(tmp_path / "guess_short.raw")
    np.zeros((4, 4, 3), np.float32).tofile(files["SHORT"])
    files["NOWHERE"] = str(tmp_path / "guess_nowhere.raw")
    extra = [files.get(a, a) for a in extra]
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--initial-flow U V W] [--warm-start | --total]" in run.stdout
    assert not [n for n in os.listdir(tmp_path) if n.startswith("o")]   # nothing was written
