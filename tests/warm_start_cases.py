"""The driver cases of the solves that start from a given displacement, written once for both backends: tests/test_gpu_warm_start.py
runs them on the GPU, tests/test_warm_start_cpu.py in a child interpreter on the host-memory stand-in of tests/cpu_device_initial.
Every function takes the package and compares the product's driver with the Python pyramid of tests/warm_start_ref.py bit for bit
(signs of zero as values: the median passes values through; NaN nowhere)."""
import numpy as np

import warm_start_ref as ws

# name -> ([z, y, x], solver settings); the frames are ws.test_pair(shape, SHIFT), the guess varying_guess(shape) round GUESS
SHIFT = (2.0, -1.5, 0.5)
GUESS = (1.5, -1.0, 0.25)
DRIVER_CASES = {
    "six_levels": ((24, 40, 48), dict(warp_levels_count=6, outer_iterations_count=5)),
    "five_planes": ((5, 64, 96), dict(warp_scale_factor=0.8, warp_levels_count=4, outer_iterations_count=4)),
    "median_three": ((20, 36, 40), dict(gaussian_sigma=0, median_radius=3, warp_levels_count=3)),
}
SMALL = ((12, 20, 26), dict(warp_levels_count=3, outer_iterations_count=2))


def varying_guess(shape):
    """GUESS plus half a voxel of a wave along every axis: a guess from host arrays that varies in space, so that a driver which copied
    it into the corner of a coarser level instead of resampling it would give other values"""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    wave = (np.sin(2.0 * np.pi * x / w), np.cos(2.0 * np.pi * y / h), np.sin(2.0 * np.pi * (x + y + 2 * z) / (w + h + 2 * d)))
    return tuple((g + 0.5 * a).astype(np.float32) for g, a in zip(GUESS, wave))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any() and bool(np.all(a == b))


def all_same(got, expected):
    return all(same(g, e) for g, e in zip(got, expected))


_references = {}


def references(name):
    """(f0, f1, guess, cold, from_guess, from_cold) of a driver case, computed once per process and never changed"""
    if name not in _references:
        shape, kw = DRIVER_CASES[name] if name in DRIVER_CASES else SMALL
        f0, f1 = ws.test_pair(shape, SHIFT)
        guess = varying_guess(shape)
        cold = ws.pyramid(f0, f1, **kw)
        _references[name] = (f0, f1, guess, cold, ws.pyramid(f0, f1, initial=guess, **kw), ws.pyramid(f0, f1, initial=cold, **kw))
        for group in _references[name][:2] + _references[name][3:]:
            for a in (group if isinstance(group, tuple) else (group,)):
                a.flags.writeable = False
    return _references[name]


def driver(pkg, shape):
    d, h, w = shape
    flow = pkg.OpticalFlow()
    flow.initialize(w, h, d)
    return flow


def check_from_arrays(pkg, name):
    shape, kw = DRIVER_CASES[name]
    f0, f1, guess, cold, from_guess, _ = references(name)
    flow = driver(pkg, shape)
    try:
        assert all_same(flow.compute(f0, f1, silent=True, **kw), cold), "initial=None is no longer the plain solve"
        assert all_same(flow.compute(f0, f1, silent=True, initial=guess, **kw), from_guess), "compute(initial=arrays)"
        # the initial flow is data: it is still there, unchanged, and the plain call never looks at it
        assert all_same(flow.initial_download(), guess)
        assert all_same(flow.compute(f0, f1, silent=True, **kw), cold), "the plain call read the initial flow"
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, initial=guess, **kw)
        assert all_same(flow.download(), from_guess), "compute_resident(initial=arrays)"
    finally:
        flow.destroy()


def check_from_flow(pkg, name):
    shape, kw = DRIVER_CASES[name]
    f0, f1, _, cold, _, from_cold = references(name)
    flow = driver(pkg, shape)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **kw)
        assert all_same(flow.download(), cold)
        flow.compute_resident(silent=True, initial="flow", **kw)
        assert all_same(flow.download(), from_cold), 'compute_resident(initial="flow")'
        assert all_same(flow.initial_download(), cold), "the copy of the held flow"
    finally:
        flow.destroy()


def check_from_trajectory(pkg, name):
    shape, kw = DRIVER_CASES[name]
    f0, f1, _, cold, _, from_cold = references(name)
    flow = driver(pkg, shape)
    try:
        flow.upload(f0, f1)
        flow.trajectory_begin()
        flow.compute_resident(silent=True, **kw)
        flow.trajectory_append()  # zero + the flow sampled where it stands: the flow itself
        flow.compute_resident(silent=True, initial="trajectory", **kw)
        assert all_same(flow.download(), from_cold), 'compute_resident(initial="trajectory")'
        flow.trajectory_end()
    finally:
        flow.destroy()


def holed_guess(shape):
    u, v, w = (a.copy() for a in ws.constant_flow(shape, GUESS))
    u[0, 0, 0] = np.nan
    w[-1, -1, -1] = np.inf
    v[shape[0] // 2, 3, 5:9] = -np.inf
    u[1, 2, 3] = np.nan
    v[1, 2, 3] = np.nan
    w[2, 2, 2] = -0.0
    return u, v, w


def check_holes(pkg):
    shape, kw = SMALL
    f0, f1 = references("small")[:2]
    guess = holed_guess(shape)
    prepared, info = ws.initial_flow(*guess)
    assert info["replaced"] == 7
    expected = ws.pyramid(f0, f1, initial=prepared, **kw)
    flow = driver(pkg, shape)
    try:
        got_info = flow.set_initial(guess)
        assert got_info.as_dict() == info, (got_info.as_dict(), info)
        held = flow.initial_download()
        assert all(np.array_equal(g.view(np.uint32), e.view(np.uint32)) for g, e in zip(held, prepared)), "the prepared guess, bit for bit"
        assert all_same(flow.compute(f0, f1, silent=True, initial=guess, **kw), expected), "a guess with holes"
    finally:
        flow.destroy()


def check_levels_one_and_zero(pkg):
    shape, kw = SMALL
    f0, f1, guess = references("small")[:3]
    flow = driver(pkg, shape)
    try:
        one = dict(kw, warp_levels_count=1)
        assert all_same(flow.compute(f0, f1, silent=True, initial=guess, **one), ws.pyramid(f0, f1, initial=guess, **one)), "one level: the copy"
        none = dict(kw, warp_levels_count=0)
        assert all_same(flow.compute(f0, f1, silent=True, initial=guess, **none), guess), "no level: the prepared initial flow"
        assert all(not a.any() for a in flow.compute(f0, f1, silent=True, **none)), "no level and no initial flow: zero"
    finally:
        flow.destroy()


def check_zeros_are_the_plain_call(pkg):
    shape, kw = SMALL
    f0, f1 = references("small")[:2]
    flow = driver(pkg, shape)
    try:
        plain = flow.compute(f0, f1, silent=True, **kw)
        zeros = flow.compute(f0, f1, silent=True, initial=ws.constant_flow(shape, (0, 0, 0)), **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, zeros)), "a guess of zeros must give the bytes of the plain call"
    finally:
        flow.destroy()


def check_refusals(pkg):
    shape, kw = SMALL
    f0, f1, guess = references("small")[:3]
    flow = driver(pkg, shape)
    try:
        for bad in ("flow", "trajectory"):  # nothing held, no trajectory
            try:
                flow.set_initial(bad)
                raise AssertionError(f"set_initial({bad!r}) with nothing to take")
            except pkg.F3dError:
                pass
        for bad in ("elsewhere", guess[:2], tuple(a[1:] for a in guess)):
            try:
                flow.set_initial(bad)
                raise AssertionError("a wrong initial was accepted")
            except ValueError:
                pass
        flow.set_initial(guess)
        flow.initial_end()
        try:
            flow.initial_download()
            raise AssertionError("a released initial flow was downloaded")
        except pkg.F3dError:
            pass
        try:
            list(flow.compute_sequence([f0, f1], cumulative=True, total=True, **kw))
            raise AssertionError("total with cumulative was accepted")
        except ValueError:
            pass
        try:
            list(flow.compute_sequence([f0, f1], warm_start=True, total=True, **kw))
            raise AssertionError("total with warm_start was accepted")
        except ValueError:
            pass
    finally:
        flow.destroy()


def sequence_frames():
    shape = SMALL[0]
    return [ws.test_pair(shape, tuple(k * s for s in SHIFT))[1] for k in range(3)]


def check_sequences(pkg):
    shape, kw = SMALL
    frames = sequence_frames()
    guess = varying_guess(shape)
    flow = driver(pkg, shape)
    try:
        # total: pair k is frame 0 -> frame k+1, started from the pair before
        first = ws.pyramid(frames[0], frames[1], initial=guess, **kw)
        second = ws.pyramid(frames[0], frames[2], initial=first, **kw)
        got = [(k, f, disp) for k, f, disp in flow.compute_sequence(frames, total=True, initial=guess, **kw)]
        assert [k for k, _, _ in got] == [0, 1] and all(disp is None for _, _, disp in got)
        assert all_same(got[0][1], first) and all_same(got[1][1], second), "compute_sequence(total=True)"
        # warm start: consecutive pairs, pair 1 started from pair 0's flow as it stands
        first = ws.pyramid(frames[0], frames[1], **kw)
        second = ws.pyramid(frames[1], frames[2], initial=first, **kw)
        got = [f for _, f, _ in flow.compute_sequence(frames, warm_start=True, **kw)]
        assert all_same(got[0], first) and all_same(got[1], second), "compute_sequence(warm_start=True)"
        # and with neither the sequence is what it was
        got = [f for _, f, _ in flow.compute_sequence(frames, **kw)]
        assert all_same(got[0], first) and all_same(got[1], ws.pyramid(frames[1], frames[2], **kw))
    finally:
        flow.destroy()
