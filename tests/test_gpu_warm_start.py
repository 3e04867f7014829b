"""Solves that start from a given displacement, on the GPU: f3d_initial_flow against its numpy restatement bit for bit
(outputs, info, and the sentinel outside the box), and the resident driver started from host arrays, from the held flow and from
the trajectory against the Python pyramid of tests/warm_start_ref.py, bit for bit.  The cases themselves are in
tests/warm_start_cases.py, which the host-memory stand-in runs too (tests/test_warm_start_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import warm_start_cases as cases
import warm_start_ref as ws

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)
BOXES = [((1, 1, 1), (9, 3, 2)), ((63, 3, 2), (70, 5, 3)), ((64, 5, 3), (80, 6, 4)), ((65, 4, 3), (96, 7, 4)), ((130, 7, 5), (140, 9, 6))]
LAYOUTS = ["finite", "nan", "one_inf", "ends", "minus_zero", "on_the_edge", "one_ulp_outside"]


def guess_of(layout, dims, rng):
    w, h, d = dims
    u, v, ww = (rng.uniform(-3, 3, size=(d, h, w)).astype(np.float32) for _ in range(3))
    x = np.broadcast_to(np.arange(w, dtype=np.float32), (d, h, w))
    if layout == "nan":
        u[:], v[:], ww[:] = np.nan, np.nan, np.nan
    elif layout == "one_inf":
        v[d // 2, h // 2, w // 2] = np.inf
    elif layout == "ends":
        u[0, 0, 0] = np.nan
        ww[-1, -1, -1] = -np.inf
    elif layout == "minus_zero":
        u[:], v[:], ww[:] = -0.0, 0.0, -0.0
    elif layout == "on_the_edge":      # x + u == W - 1 exactly: still inside
        u[:] = np.float32(w - 1) - x
        v[:], ww[:] = 0.0, 0.0
    elif layout == "one_ulp_outside":  # the next float after W - 1 (or after 0 downwards, for W = 1): outside
        u[:] = np.nextafter(np.float32(w - 1), np.float32(np.inf)) - x if w > 1 else -np.float32(1e-45)
        v[:], ww[:] = 0.0, 0.0
    return u, v, ww


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("dims,cdims", BOXES, ids=["x".join(map(str, b[0])) for b in BOXES])
def test_initial_flow_equals_the_restatement_bit_for_bit(f3d, dims, cdims):
    fn = f3d._initial_entry()
    w, h, d = dims
    wc, hc, dc = cdims
    rng = np.random.default_rng(28)
    box = f3d.Containers(wc, hc, dc)
    try:
        for layout in LAYOUTS:
            guess = guess_of(layout, dims, rng)
            expected, info = ws.initial_flow(*guess)
            if layout == "one_ulp_outside":
                assert info["leaving"] == info["voxels"]
            if layout == "on_the_edge":
                assert info["leaving"] == 0
            for in_place in (False, True):
                held = []
                for a in guess:
                    c = np.full((dc, hc, wc), SENTINEL, np.float32)
                    c[:d, :h, :w] = a
                    held.append(c)
                ins = [box.new(c) for c in held]
                outs = ins if in_place else [box.new(np.full((dc, hc, wc), SENTINEL, np.float32)) for _ in range(3)]
                box.set_current()
                got_info = f3d.InitialInfo()
                f3d.check(fn(*ins, *outs, w, h, d, C.byref(got_info)), "f3d_initial_flow")
                assert got_info.as_dict() == info, (layout, in_place, got_info.as_dict(), info)
                assert bits(np.float32(got_info.max_abs)) == bits(info["max_abs"])
                for p, e, c in zip(outs, expected, held):
                    got = box.download(p, cdims)
                    assert np.array_equal(bits(got[:d, :h, :w]), bits(e)), (layout, in_place)
                    outside = np.ones((dc, hc, wc), bool)
                    outside[:d, :h, :w] = False
                    assert np.all(got[outside] == SENTINEL), (layout, in_place, "the padding was written")
                if not in_place:  # the inputs are only read
                    for p, c in zip(ins, held):
                        assert np.array_equal(bits(box.download(p, cdims)), bits(c)), (layout, "an input was written")
                # without info the call only enqueues, and stores the same
                f3d.check(fn(*ins, *outs, w, h, d, None), "f3d_initial_flow")
                f3d.sync()
                assert np.array_equal(bits(box.download(outs[0], cdims)[:d, :h, :w]), bits(expected[0]))
                box.free()
    finally:
        box.free()


def test_initial_flow_refuses_what_it_cannot_do(f3d):
    fn = f3d._initial_entry()
    box = f3d.Containers(16, 4, 3)
    try:
        a, b, c, o = (box.new(np.zeros((3, 4, 16), np.float32)) for _ in range(4))
        box.set_current()
        bad = [((0, b, c, a, b, c), (16, 4, 3)), ((a, 0, c, a, b, c), (16, 4, 3)), ((a, b, 0, a, b, c), (16, 4, 3)),
               ((a, b, c, 0, b, c), (16, 4, 3)), ((a, b, c, a, 0, c), (16, 4, 3)), ((a, b, c, a, b, 0), (16, 4, 3)),
               ((a, b, c, a, b, c), (0, 4, 3)), ((a, b, c, a, b, c), (16, 0, 3)), ((a, b, c, a, b, c), (16, 4, 0)),
               ((a, b, c, a, b, c), (17, 4, 3)), ((a, b, c, a, b, c), (16, 5, 3)), ((a, b, c, a, b, c), (16, 4, 4)),
               ((a, b, c, b, a, c), (16, 4, 3)), ((a, b, c, o, o, c), (16, 4, 3))]
        for ptrs, dims in bad:
            assert fn(*ptrs, *dims, None) != 0, (ptrs, dims)
            assert b"f3d_initial_flow" in f3d.hip().f3d_last_error()
        assert fn(a, b, c, a, b, c, 16, 4, 3, None) == 0
        f3d.sync()
    finally:
        box.free()


def test_initial_flow_of_volumes_from_anywhere(f3d):
    guess = cases.holed_guess(cases.SMALL[0])
    expected, info = ws.initial_flow(*guess)
    got, got_info = f3d.initial_flow(*guess)
    assert got_info.as_dict() == info
    assert all(np.array_equal(bits(g), bits(e)) for g, e in zip(got, expected))


@pytest.mark.parametrize("name", list(cases.DRIVER_CASES))
def test_driver_from_host_arrays_equals_the_pyramid(f3d, name):
    cases.check_from_arrays(f3d, name)


@pytest.mark.parametrize("name", list(cases.DRIVER_CASES))
def test_driver_from_the_held_flow_equals_the_pyramid(f3d, name):
    cases.check_from_flow(f3d, name)


@pytest.mark.parametrize("name", list(cases.DRIVER_CASES))
def test_driver_from_the_trajectory_equals_the_pyramid(f3d, name):
    cases.check_from_trajectory(f3d, name)


def test_driver_with_one_level_and_with_none(f3d):
    cases.check_levels_one_and_zero(f3d)


def test_driver_from_a_guess_with_holes(f3d):
    cases.check_holes(f3d)


def test_driver_on_the_schedule_without_weights_first(f3d, monkeypatch):
    monkeypatch.setenv("F3D_WEIGHTS_FIRST", "0")
    cases.check_from_arrays(f3d, "six_levels")


def test_a_guess_of_zeros_gives_the_bytes_of_the_plain_call(f3d):
    cases.check_zeros_are_the_plain_call(f3d)


def test_driver_refusals(f3d):
    cases.check_refusals(f3d)


def test_sequences_total_and_warm_start_equal_the_chain_of_restatements(f3d):
    cases.check_sequences(f3d)


def test_the_guess_lowers_the_residual_the_first_level_meets(f3d):
    """With level statistics on, the residual before the solve at the first level is lower from the guess (5, -3, 2), which is off by
    one voxel per axis, than from zero, which is off by (6, -4, 3)."""
    f0, f1 = ws.test_pair()
    guess = ws.constant_flow(f0.shape, ws.PAIR_GUESS)
    d, h, w = f0.shape
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.set_level_stats(True)
        flow.upload(f0, f1)
        kw = dict(warp_levels_count=6, outer_iterations_count=2)
        flow.compute_resident(silent=True, **kw)
        cold = flow.level_stats()
        flow.compute_resident(silent=True, initial=guess, **kw)
        warm = flow.level_stats()
        assert len(cold) == len(warm) == 6 and cold[0]["level"] == warm[0]["level"] == 5
        print("residual before the first level's solve: cold", cold[0]["residual_rms"], "from the guess", warm[0]["residual_rms"])
        assert warm[0]["residual_rms"] < cold[0]["residual_rms"]
    finally:
        flow.destroy()


def run_flow3d(tmp_path, frames, tag, extra, kw):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "cuda-flow3d_amd", "bin", "flow3d")
    d, h, w = frames[0].shape
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"frame{i}.raw"))
        f.tofile(paths[-1])
    prefix = str(tmp_path / tag)
    run = subprocess.run([exe, "--dims", str(w), str(h), str(d), "--f32", "--frames", *paths, "--out", prefix, "--silent", "--levels",
                          str(kw["warp_levels_count"]), "--outer", str(kw["outer_iterations_count"])] + extra, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-1500:], run.stderr[-1500:])
    pairs = len(frames) - 1

    def read(k):
        name = f"{prefix}_{k}" if pairs > 1 else prefix
        return tuple(open(f"{name}_flow-{c}-{w}-{h}-{d}.raw", "rb").read() for c in "uvw")

    return [read(k) for k in range(pairs)], run.stdout


@pytest.mark.parametrize("option,python", [("--total", dict(total=True)), ("--warm-start", dict(warm_start=True))])
def test_flow3d_total_and_warm_start_write_the_flows_of_the_python_calls(f3d, tmp_path, option, python):
    shape, kw = cases.SMALL
    frames = cases.sequence_frames()
    written, text = run_flow3d(tmp_path, frames, "seq", [option], kw)
    flow = cases.driver(f3d, shape)
    try:
        expected = [f for _, f, _ in flow.compute_sequence(frames, **python, **kw)]
    finally:
        flow.destroy()
    assert len(written) == len(expected) == 2
    for got, exp in zip(written, expected):
        assert all(g == e.tobytes() for g, e in zip(got, exp)), option
    # pair 1 started from pair 0's flow, and said what it found there
    assert text.count("initial flow: 0 replaced") == 1, text[-1500:]
    # with two frames both options are allowed and do nothing
    alone, text = run_flow3d(tmp_path, frames[:2], "two", [option], kw)
    plain, _ = run_flow3d(tmp_path, frames[:2], "plain", [], kw)
    assert alone == plain and "initial flow:" not in text


def test_flow3d_initial_flow_writes_the_flow_of_the_python_call(f3d, tmp_path):
    shape, kw = cases.SMALL
    frames = cases.sequence_frames()[:2]
    guess = cases.holed_guess(shape)
    files = []
    for name, a in zip("uvw", guess):
        files.append(str(tmp_path / f"guess-{name}.raw"))
        a.tofile(files[-1])
    written, text = run_flow3d(tmp_path, frames, "guess", ["--initial-flow", *files], kw)
    flow = cases.driver(f3d, shape)
    try:
        expected = flow.compute(frames[0], frames[1], silent=True, initial=guess, **kw)
    finally:
        flow.destroy()
    assert all(g == e.tobytes() for g, e in zip(written[0], expected))
    info = ws.initial_flow(*guess)[1]
    assert f"initial flow: {info['replaced']} replaced, {info['leaving']} leaving, max |.| 1.5" in text, text[-1500:]
