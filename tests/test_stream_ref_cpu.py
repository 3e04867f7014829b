"""The oracle's resampling, convolution and warp against their definitions in binary64 (tests/stream_ref.py), on the CPU.

tests/test_gpu_stream_routes.py asks the device for the oracle's bits; this file asks whether the oracle computes the right thing, within
the float32 rounding bounds derived in tests/stream_ref.py -- bounds far below the error of a wrong cell, a wrong fraction or a tap vector
read backwards, which is of the order of the data itself (the last tests here measure that margin).  The oracle's worst ratio to each
bound is printed; LABBOOK.md records what it was when the bounds were chosen."""
import numpy as np
import pytest

import stream_ref as sr
from conftest import bit_same

AXES = [0, 1, 2]
SPACINGS = [(0.7, 3.0, 1.3), (2.0, 1.0, 0.7)]


def dims_along(axis, n, others=(6, 5)):
    d = list(others)
    d.insert(axis, n)
    return tuple(d)   # (W, H, D)


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("n,m", sr.RATIOS)
def test_oracle_resampling_is_the_mean_over_the_window(oracle, n, m, axis):
    rng = np.random.default_rng(100 * n + m + axis)
    W, H, D = dims_along(axis, n)
    ow, oh, od = dims_along(axis, m)
    src = rng.uniform(-5, 5, (D, H, W)).astype(np.float32)
    got = np.full((od, oh, ow), np.nan, np.float32)
    oracle.resample_axis(src, got, (ow, oh, od), n, axis)
    err, bound = sr.worst(got, sr.resample_axis(src, m, axis)), sr.resample_bound(n, m, float(np.abs(src).max()))
    print(f"resample {n}->{m} axis {axis}: {err / bound * sr.C_RESAMPLE:.3f} of u (m + cnt) max|s|")
    assert err <= bound


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("R", sr.RADII)
def test_oracle_convolution_is_the_zero_padded_sum(oracle, R, axis):
    """with taps that are no palindrome; the axis is shorter than the radius for the larger radii"""
    rng = np.random.default_rng(200 + 10 * R + axis)
    dims = dims_along(axis, 13, (7, 4))
    W, H, D = dims
    taps = sr.asym_taps(R)
    src = rng.uniform(-3, 3, (D, H, W)).astype(np.float32)
    got = np.full_like(src, np.nan)
    oracle.conv_axis(got, src, dims, R, taps, axis)
    err, bound = sr.worst(got, sr.conv_axis(src, taps, axis)), sr.conv_bound(taps, float(np.abs(src).max()))
    print(f"conv R {R} axis {axis}: {err / bound * sr.C_CONV:.3f} of u (2R + 2) sum|k| max|s|")
    assert err <= bound


@pytest.mark.parametrize("h", SPACINGS)
@pytest.mark.parametrize("dims", [(13, 9, 7), (9, 7, 16), (1, 1, 1), (1, 6, 5), (6, 1, 5), (6, 5, 1)])
def test_oracle_warp_is_the_trilinear_sample(oracle, dims, h):
    rng = np.random.default_rng(300 + sum(dims))
    W, H, D = dims
    (f0, f1, u, v, w), planted, share = sr.warp_case(rng, dims, h, plant=min(dims) > 4)
    if min(dims) > 4:
        assert 0.2 <= share <= 0.8, share
        assert {e for *_, e in planted} == {"f0", "in"}
    got = oracle.warp(f0, f1, u, v, w, dims, h)
    inside = sr.warp_coordinates(u, v, w, h)[3]
    for z, y, x, expect in planted:
        assert inside[z, y, x] == (expect == "in"), (z, y, x, expect)
    assert bit_same(got[~inside], f0[~inside])
    err, bound = sr.worst(got, sr.warp(f0, f1, u, v, w, h)), sr.warp_bound(float(np.abs(f1).max()))
    print(f"warp {dims} h {h}: {err / bound * sr.C_WARP:.3f} of u max|f1|")
    assert err <= bound


def test_oracle_z_pass_on_a_window_is_the_whole_volume_cut(oracle):
    """input and output containers with z_base of their own; nothing else is written"""
    rng = np.random.default_rng(5)
    for n, m, (z_lo, z_hi) in [(23, 9, (2, 6)), (9, 23, (5, 7)), (17, 17, (4, 10)), (50, 7, (1, 3))]:
        src = rng.uniform(-5, 5, (n, 5, 6)).astype(np.float32)
        whole = np.full((m, 5, 6), np.nan, np.float32)
        oracle.resample_axis(src, whole, (6, 5, m), n, 2)
        delta = np.float32(n) / np.float32(m)
        lo, hi = int(np.floor(np.float32(z_lo) * delta)), min(n, int(np.ceil(np.float32(z_hi) * delta)))
        part = np.ascontiguousarray(src[lo:hi])
        out = np.full((z_hi - z_lo + 2, 5, 6), np.nan, np.float32)
        oracle.resample_axis(part, out, (6, 5, m), n, 2, oracle.Geom(5, 6, lo, lo, hi), oracle.Geom(5, 6, z_lo - 1, z_lo, z_hi))
        assert bit_same(out[1:-1], whole[z_lo:z_hi]) and np.isnan(out[0]).all() and np.isnan(out[-1]).all()


# ---- the margin: what a wrong kernel would miss the bounds by ------------------------------------------------------------------------

def test_a_reversed_tap_vector_misses_the_bound_by_orders_of_magnitude():
    rng = np.random.default_rng(6)
    src = rng.uniform(-3, 3, (5, 6, 40)).astype(np.float32)
    for R in sr.RADII:
        taps = sr.asym_taps(R)
        wrong = sr.worst(sr.conv_axis(src, taps[::-1], 0), sr.conv_axis(src, taps, 0))
        assert wrong > 1e4 * sr.conv_bound(taps, 3.0), R


def test_a_wrong_cell_or_fraction_misses_the_resampling_bound_by_orders_of_magnitude():
    rng = np.random.default_rng(7)
    for n, m in sr.RATIOS:
        if n == 1 or m == 1:
            continue   # one cell or one window: a rotation of the cells changes nothing
        src = rng.uniform(-5, 5, (3, 4, n)).astype(np.float32)
        shifted = np.roll(src, 1, axis=2)   # every window one cell off
        wrong = sr.worst(sr.resample_axis(shifted, m, 0), sr.resample_axis(src, m, 0))
        assert wrong > 1e3 * sr.resample_bound(n, m, 5.0), (n, m)


def test_a_neighbouring_cell_misses_the_warp_bound_by_orders_of_magnitude():
    rng = np.random.default_rng(8)
    h = SPACINGS[0]
    (f0, f1, u, v, w), _, _ = sr.warp_case(rng, (13, 9, 7), h)
    wrong = sr.worst(sr.warp(f0, np.roll(f1, 1, axis=2), u, v, w, h), sr.warp(f0, f1, u, v, w, h))
    assert wrong > 1e4 * sr.warp_bound(255.0)
