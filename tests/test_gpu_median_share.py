"""k_median_share, the 5^3 median that forms every merged plane pair once (kept in LDS) and builds its plane lists from sorted
y-columns shared between the lanes of a workgroup: forced (F3D_MEDIAN_PAIR=3) and as the default (variable unset).

Against the oracle with plateaus and zeros everywhere (ties), bit for bit against k_median_keep (F3D_MEDIAN_PAIR=2) on data
without mixed-sign zeros, on shapes that cross every edge of the data movement: widths around the 64-lane tile and its 68-column
footprint, heights around the 4-row tile, depths that end the four-step unroll at every position, chunks of several steps, slab
windows whose container holds nothing beyond the two halo planes, and batches of one to three volumes."""
import ctypes as C

import numpy as np
import pytest

from conftest import bit_same, box_in_container, same
from test_gpu_kernels import Dev, _dev_array

pytestmark = pytest.mark.gpu

WIDTHS = (3, 5, 63, 64, 65, 68, 130)
HEIGHTS = (3, 4, 5, 9)
DEPTHS = (3, 4, 5, 6, 7, 8, 9, 13, 19)
VARIANTS = ("3", None)


def select(monkeypatch, variant):
    if variant is None:
        monkeypatch.delenv("F3D_MEDIAN_PAIR", raising=False)
    else:
        monkeypatch.setenv("F3D_MEDIAN_PAIR", variant)


def volume(rng, dims, cdims=None):
    """the data of the existing median tests: uniform values with plateaus of 0.5 and exact (+0) zeros"""
    W, H, D = dims
    inp = box_in_container(rng, dims, cdims or dims, -2, 2)
    inp[:D, :H, :W][rng.random((D, H, W)) < 0.3] = 0.5
    inp[:D, :H, :W][rng.random((D, H, W)) < 0.1] = 0.0
    return inp


def run(f3d, dev, pin, dims, slab=None):
    W, H, D = dims
    pout = dev.out()
    f3d.check(f3d.hip().f3d_median(pin, W, H, D, 5, pout, C.byref(slab) if slab else None))
    return dev.get(pout)


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_shapes_against_the_oracle_and_the_kept_planes_kernel(f3d, oracle, W, H, monkeypatch):
    for D in DEPTHS:
        dims = (W, H, D)
        rng = np.random.default_rng(1000 * W + 100 * H + D)
        inp = volume(rng, dims)
        exp = oracle.median(inp, dims, 5)
        dev = Dev(f3d, dims)
        try:
            pin = dev.put(inp)
            select(monkeypatch, "2")
            kept = run(f3d, dev, pin, dims)
            for variant in VARIANTS:
                select(monkeypatch, variant)
                got = run(f3d, dev, pin, dims)
                assert same(got, exp), (dims, variant)
                assert bit_same(got, kept), (dims, variant)
        finally:
            dev.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dims,cdims", [((200, 150, 41), (200, 150, 41)), ((200, 150, 39), (208, 152, 40)), ((37, 21, 9), (64, 32, 16)),
                                        ((131, 70, 30), (192, 72, 32))])
def test_long_chunks(f3d, oracle, dims, cdims, variant, monkeypatch):
    """Volumes with enough workgroups for the launch model to choose chunks of four and five steps (200 x 150: chunks of 8 and
    10 planes), so the march goes round its unroll; box in the corner of a NaN-filled container."""
    rng = np.random.default_rng(41)
    W, H, D = dims
    inp = volume(rng, dims, cdims)
    exp = oracle.median(inp, dims, 5)
    dev = Dev(f3d, cdims)
    try:
        pin = dev.put(inp)
        select(monkeypatch, "2")
        kept = run(f3d, dev, pin, dims)
        select(monkeypatch, variant)
        got = run(f3d, dev, pin, dims)
        assert same(got[:D, :H, :W], exp[:D, :H, :W])
        assert bit_same(got[:D, :H, :W], kept[:D, :H, :W])
        # nothing outside the box is written: both outputs started from the same fill
        assert got.tobytes() == kept.tobytes()
    finally:
        dev.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dims,window", [((66, 10, 31), (0, 9)), ((66, 10, 31), (7, 24)), ((66, 10, 31), (20, 31)), ((20, 12, 17), (0, 5)),
                                         ((20, 12, 17), (6, 11)), ((20, 12, 17), (12, 17)), ((130, 9, 19), (0, 1)), ((130, 9, 19), (9, 10)),
                                         ((130, 9, 19), (18, 19)), ((200, 150, 41), (3, 38))])
def test_slab_windows(f3d, oracle, dims, window, variant, monkeypatch):
    """A window at the bottom, in the middle and at the top of a volume; the container holds the window and its two halo planes
    and nothing else, so a plane fetched from beyond them is a read outside the container."""
    select(monkeypatch, variant)
    rng = np.random.default_rng(43)
    W, H, D = dims
    inp = volume(rng, dims)
    exp = oracle.median(inp, dims, 5)
    z_lo, z_hi = window
    z_base, top = max(0, z_lo - 2), min(D, z_hi + 2)
    dev = Dev(f3d, (W, H, top - z_base))
    try:
        pin = dev.put(np.ascontiguousarray(inp[z_base:top]))
        slab = f3d.Slab(z_base, z_lo, z_hi)
        got = run(f3d, dev, pin, dims, slab)
        assert same(got[z_lo - z_base:z_hi - z_base], exp[z_lo:z_hi])
        select(monkeypatch, "2")
        kept = run(f3d, dev, pin, dims, slab)
        assert got.tobytes() == kept.tobytes()
    finally:
        dev.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("dims,cdims,window", [((37, 21, 9), (64, 32, 16), None), ((130, 9, 19), (130, 9, 19), None),
                                               ((20, 12, 17), (24, 12, 17), (3, 11)), ((200, 150, 39), (200, 150, 39), None)])
def test_batches_equal_single_launches(f3d, oracle, dims, cdims, window, count, variant, monkeypatch):
    """f3d_median_n on one, two and three volumes against as many single launches (pinned to the oracle here as well)."""
    select(monkeypatch, variant)
    hip = f3d.hip()
    rng = np.random.default_rng(47 + count)
    W, H, D = dims
    z_lo, z_hi = window or (0, D)
    slab = C.byref(f3d.Slab(0, z_lo, z_hi)) if window else None
    vols = [volume(rng, dims, cdims) for _ in range(count)]
    dev = Dev(f3d, cdims)
    try:
        pin = [dev.put(v) for v in vols]
        one = [dev.out() for _ in range(count)]
        many = [dev.out() for _ in range(count)]
        for i in range(count):
            f3d.check(hip.f3d_median(pin[i], W, H, D, 5, one[i], slab))
        f3d.check(hip.f3d_median_n(_dev_array(pin), count, W, H, D, 5, _dev_array(many), slab))
        for i in range(count):
            got = dev.get(many[i])
            assert got.tobytes() == dev.get(one[i]).tobytes(), i
            assert same(got[z_lo:z_hi, :H, :W], oracle.median(vols[i], dims, 5)[z_lo:z_hi, :H, :W]), i
    finally:
        dev.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_sign_zeros_keep_their_value(f3d, oracle, variant, monkeypatch, capsys):
    """Windows that hold both -0 and +0: the value is the oracle's (the zeros compare equal); the sign of a zero result is the one
    thing the kernels may disagree on, so it is counted and printed, not asserted."""
    dims = (70, 9, 23)
    rng = np.random.default_rng(53)
    W, H, D = dims
    inp = volume(rng, dims)
    inp[rng.random((D, H, W)) < 0.25] = -0.0
    inp[rng.random((D, H, W)) < 0.25] = 0.0
    exp = oracle.median(inp, dims, 5)
    dev = Dev(f3d, dims)
    try:
        pin = dev.put(inp)
        select(monkeypatch, variant)
        got = run(f3d, dev, pin, dims)
        select(monkeypatch, "2")
        kept = run(f3d, dev, pin, dims)
        assert same(got, exp) and same(kept, exp)
        with capsys.disabled():
            print(f"\nmixed-sign zeros, F3D_MEDIAN_PAIR={variant}: {int((got.view(np.uint32) != kept.view(np.uint32)).sum())} of "
                  f"{int((exp == 0).sum())} zero results differ in sign from k_median_keep, "
                  f"{int((got.view(np.uint32) != exp.view(np.uint32)).sum())} from the oracle")
    finally:
        dev.close()
