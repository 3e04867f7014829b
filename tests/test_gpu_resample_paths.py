"""The routes of the x resampling pass on the MI355X (f3d_resample_x / f3d_resample_x_n).

The launcher takes k_resample_x_rows (a wave walks several rows, windows held in registers, rows double-buffered in LDS) for rows of
up to 1024 floats resampled to up to 1024 outputs, k_resample_x_lds for longer staged rows (up to 2048 floats) and k_resample<0> beyond
that or where a row is not 16-byte aligned.  Every route must leave the bits of k_resample<0> -- reached here by handing the same
launch an output that starts 4 bytes into its container, which no staged route accepts -- and of the oracle's x pass.  Boxes sit in
NaN-poisoned containers; nothing outside the box (or the slab window) may be written."""
import ctypes as C

import numpy as np
import pytest

from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu

# source width -> output width
WIDTHS = [
    (37, 5),       # windows of 8-9 cells
    (64, 61),      # windows of 1-2 cells
    (65, 64),
    (130, 124),
    (5, 37),       # up-sampling: windows of one cell (cnt == 1) and of two
    (61, 64),
    (700, 520),    # more than 512 outputs: the instantiation with 16 outputs and 4 pieces per lane
    (1030, 64),    # a staged row beyond the row-walking kernel's 1024 floats: k_resample_x_lds
]


def _dev_array(ptrs):
    return (C.c_uint64 * len(ptrs))(*ptrs)


class Dev:
    def __init__(self, f3d, cdims):
        self.f3d, self.cdims = f3d, cdims
        self.cont = f3d.Containers(*cdims)
        self.cont.alloc(fill=0xFF)
        self.cont.set_current()

    def put(self, host):
        p = self.cont.new()
        self.cont.upload(p, host)
        return p

    def out(self):
        return self.cont.new()

    def get(self, p):
        self.f3d.sync()
        return self.cont.download(p, self.cdims)

    def close(self):
        self.f3d.sync()
        self.cont.free()


def check_x_pass(f3d, oracle, in_w, out_w, H, D, count, window=None, seed=1):
    """f3d_resample_x[_n] on `count` volumes against the oracle and against the generic kernel (unaligned output)"""
    hip = f3d.hip()
    cw = max(in_w, out_w) + 4          # room for the output shifted by one column
    cdims = (cw, H, D)
    rng = np.random.default_rng(seed)
    z_lo, z_hi = window or (0, D)
    slab_obj = f3d.Slab(0, z_lo, z_hi) if window else None
    slab = C.byref(slab_obj) if window else None
    vols = [box_in_container(rng, (in_w, H, D), cdims, -2, 2) for _ in range(count)]
    dev = Dev(f3d, cdims)
    try:
        pin = [dev.put(v) for v in vols]
        pout = [dev.out() for _ in range(count)]
        pref = [dev.out() for _ in range(count)]
        if count == 1:
            f3d.check(hip.f3d_resample_x(pin[0], pout[0], out_w, H, D, in_w, slab))
            f3d.check(hip.f3d_resample_x(pin[0], pref[0] + 4, out_w, H, D, in_w, slab))
        else:
            f3d.check(hip.f3d_resample_x_n(_dev_array(pin), _dev_array(pout), count, out_w, H, D, in_w, slab))
            f3d.check(hip.f3d_resample_x_n(_dev_array(pin), _dev_array([p + 4 for p in pref]), count, out_w, H, D, in_w, slab))
        for i in range(count):
            exp = np.full_like(vols[i], np.nan)
            oracle.resample_axis(vols[i], exp, (out_w, H, D), in_w, 0)
            got, ref = dev.get(pout[i]), dev.get(pref[i])
            assert bit_same(got[z_lo:z_hi, :, :out_w], exp[z_lo:z_hi, :, :out_w]), f"volume {i}: differs from the oracle"
            assert bit_same(got[z_lo:z_hi, :, :out_w], ref[z_lo:z_hi, :, 1:out_w + 1]), f"volume {i}: differs from k_resample<0>"
            untouched = np.ones(got.shape, bool)
            untouched[z_lo:z_hi, :, :out_w] = False
            assert np.isnan(got[untouched]).all(), f"volume {i}: written outside the box"
            assert bit_same(dev.get(pin[i]), vols[i])
    finally:
        dev.close()


@pytest.mark.parametrize("in_w,out_w", WIDTHS)
def test_x_pass_widths(f3d, oracle, in_w, out_w):
    check_x_pass(f3d, oracle, in_w, out_w, H=13, D=3, count=3)


@pytest.mark.parametrize("H", [1, 5, 13])
@pytest.mark.parametrize("count", [1, 2, 3])
def test_x_pass_heights_and_batches(f3d, oracle, H, count):
    """heights that are not multiples of the four rows of a workgroup; one volume (f3d_resample_x), two and three (f3d_resample_x_n)"""
    check_x_pass(f3d, oracle, 130, 124, H=H, D=4, count=count, seed=H * 10 + count)


def test_x_pass_beyond_the_staging_limit(f3d, oracle):
    """2049 floats do not fit the staged row of any LDS route: k_resample<0> itself"""
    check_x_pass(f3d, oracle, 2049, 1947, H=3, D=2, count=1)


def test_x_pass_under_a_slab_window(f3d, oracle):
    check_x_pass(f3d, oracle, 65, 64, H=13, D=9, count=2, window=(2, 7))


@pytest.mark.parametrize("D,rows_per_wave", [(182, 2), (364, 4), (728, 8)])
def test_x_pass_walks_several_rows_per_wave(f3d, oracle, D, rows_per_wave):
    """The launcher gives a wave 2, 4 or 8 rows once a launch has 32768, 65536 or 131072 rows: 181 rows per plane (no multiple of the
    rows of a workgroup, so the last workgroup of a plane has idle waves and a wave with a short walk) on narrow rows."""
    assert 181 * D >= 16384 * rows_per_wave and (rows_per_wave == 8 or 181 * D < 32768 * rows_per_wave)
    check_x_pass(f3d, oracle, 37, 5, H=181, D=D, count=1)
