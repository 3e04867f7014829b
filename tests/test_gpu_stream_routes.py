"""Every launch route, tile seam and z-window of the streaming passes of the pyramid loop on the MI355X: the y and z resampling passes,
the Gaussian launchers, warp and add (csrc/f3d_stream_ops.hip, csrc/f3d_gauss.hip), called directly.

The bar is the suite's: the oracle's bits on the box or window.  Beyond that, every output lives in a container poisoned with 0xFF bytes
and every word of it outside the box or window must still be poison afterwards, and every input must be unchanged: one helper,
Dev.only_box_written, states "box equal, rest untouched" for every test here.  A windowed expectation is the oracle's whole-volume result
cut to the window (tests/test_stream_ref_cpu.py checks that the oracle's own windowed z pass is that cut).  A handful of cases are also held
against the binary64 statements of tests/stream_ref.py under the rounding bounds derived there.

 * resampling: k_resample_x4<1|2> with every tail shape W % 4 and, through a pointer 4 bytes into its container (output, then input),
   the generic k_resample<1|2>; strong and mild down-sampling, identity, mild and strong up-sampling, one source cell, one output;
   one, two and three volumes; the y pass on a window with z_base > 0; the z pass between containers with different z_base that hold
   exactly the planes needed; the launcher's refusal of an input container one plane short.
 * Gaussian: taps that are no palindrome (k[R - j] and k[R + j] differ), R = 1, 2, 3, 6, 10, 25 (both compiled radii, the generic road,
   the 51-tap limit); k_gauss_xy over two and three tile rows and columns and on boxes smaller than the radius; the z march over two and
   three chunks (premise asserted from the launcher's own arithmetic), on a window, and with fewer planes than the radius.
 * warp: slab windows with all six volumes in slab containers whose planes the flow provably never leaves, spacings with inexact
   reciprocals, planted edge landings per component, boxes with an axis of one cell, frame_0 as the output.
 * add: a window with z_base > 0 inside a wider and taller container."""
import ctypes as C
import math

import numpy as np
import pytest

import stream_ref as sr
from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)


def poison(shape):
    return np.full(shape, 0xFFFFFFFF, np.uint32).view(np.float32)


def _dev_array(ptrs):
    return (C.c_uint64 * len(ptrs))(*ptrs)


class Dev:
    """Equal containers [cd, ch, cw] on the device; remembers what every one of them must hold."""

    def __init__(self, f3d, cw, ch, cd):
        self.f3d, self.cdims = f3d, (cw, ch, cd)
        self.cont = f3d.Containers(cw, ch, cd)
        self.cont.alloc(fill=0xFF)
        self.cont.set_current()
        self.image = {}

    def out(self):
        p = self.cont.new()
        self.image[p] = poison(self.cdims[::-1])
        return p

    def put(self, planes, shift=0):
        """planes [<= cd, ch, cw] into the first planes of a poisoned container, `shift` columns to the right (the last `shift`
        columns of `planes` are padding and fall off)"""
        p = self.out()
        img = self.image[p]
        img[:planes.shape[0], :, shift:] = planes[:, :, :planes.shape[2] - shift]
        self.cont.upload(p, img)
        return p

    def get(self, p):
        self.f3d.sync()
        return self.cont.download(p, self.cdims)

    def unchanged(self, ptrs, what=""):
        for p in ptrs:
            assert bit_same(self.get(p), self.image[p]), f"{what}: a container that was only read has changed"

    def only_box_written(self, p, exp, planes, H, W, x0=0, what=""):
        """BOX EQUAL, REST UNTOUCHED: container p holds exp [planes, H, W] at planes `planes` (a slice, container coordinates), rows
        [0, H), columns [x0, x0 + W), bit for bit, and every other word of it is what it was before the launch."""
        got = self.get(p)
        want = self.image[p].copy()
        want[planes, :H, x0:x0 + W] = exp
        diff = got.view(np.uint32) != want.view(np.uint32)
        if diff.any():
            box = np.zeros(diff.shape, bool)
            box[planes, :H, x0:x0 + W] = True
            z, y, x = (int(i) for i in np.argwhere(diff)[0])
            raise AssertionError(f"{what}: {int((diff & box).sum())} words of the box differ and {int((diff & ~box).sum())} words outside it "
                                 f"were written; first at plane {z} row {y} column {x}: {got[z, y, x]!r}, expected {want[z, y, x]!r}")
        self.image[p] = want

    def close(self):
        self.f3d.sync()
        self.cont.free()


def refused(f3d, status, *words):
    msg = f3d.hip().f3d_last_error() or b""
    assert status != 0 and msg, "the launcher accepted the call"
    for w in words:
        assert w.encode() in msg, msg
    return True


# ---- y and z resampling passes -------------------------------------------------------------------------------------------------------

VARIANTS = [(0, 0, "k_resample_x4"), (0, 1, "k_resample, output 4 bytes in"), (1, 0, "k_resample, input 4 bytes in")]


def z_source_planes(n, m, z_lo, z_hi):
    """the source planes output planes [z_lo, z_hi) read, with the float32 quotient the launcher forms"""
    delta = np.float32(n) / np.float32(m)
    return int(np.floor(np.float32(z_lo) * delta)), min(n, int(np.ceil(np.float32(z_hi) * delta)))


def check_pass(f3d, oracle, axis, n, m, W, other, count, window=None, seed=0, exact=False):
    """f3d_resample_{y,z}[_n] of `count` volumes from n to m cells along `axis` (1 = y, 2 = z), the other two extents W and `other`, on
    each of VARIANTS.  y pass: window = (z_base, z_lo, z_hi), containers hold the planes [z_base, z_hi] (one spare).  z pass:
    window = (z_base of the output, z_lo, z_hi); the input containers hold exactly the planes the window reads, from their own z_base."""
    hip = f3d.hip()
    name = "f3d_resample_" + "xyz"[axis]
    rng = np.random.default_rng(1000 * axis + 100 * n + m + seed)
    if axis == 1:
        src_dims, dst_dims = (W, n, other), (W, m, other)
        zb_out, z_lo, z_hi = window or (0, 0, other)
        zb_in, cd = zb_out, z_hi - zb_out + 1
        slab_in, slab = None, (f3d.Slab(zb_out, z_lo, z_hi) if window else None)
    else:
        src_dims, dst_dims = (W, other, n), (W, other, m)
        zb_out, z_lo, z_hi = window or (0, 0, m)
        if window:
            zb_in, top = z_source_planes(n, m, z_lo, z_hi)
            cd = top - zb_in
            assert z_hi - zb_out <= cd, "the output window must fit the depth of the input container"
            slab_in, slab = f3d.Slab(zb_in, zb_in, top), f3d.Slab(zb_out, z_lo, z_hi)
        else:
            zb_in, cd, slab_in, slab = 0, max(n, m) + 1, None, None
    cw, ch = W + 4, max(src_dims[1], dst_dims[1]) + 1
    ow, oh, od = dst_dims
    srcs = [box_in_container(rng, src_dims, (cw, ch, src_dims[2]), -5, 5) for _ in range(count)]
    exps = []
    for s in srcs:
        e = np.full((od, ch, cw), np.nan, np.float32)
        oracle.resample_axis(s, e, dst_dims, n, axis)
        exps.append(e[z_lo:z_hi, :oh, :ow])
    planes = slice(z_lo - zb_out, z_hi - zb_out)
    ref = lambda s: C.byref(s) if s is not None else None
    dev = Dev(f3d, cw, ch, cd)
    try:
        for din, dout, kernel in VARIANTS:
            what = f"{name} {n}->{m}, {W} wide, {count} volumes, {kernel}"
            pin = [dev.put(s[zb_in:zb_in + cd], shift=din) for s in srcs]
            pout = [dev.out() for _ in range(count)]
            a, b = [p + 4 * din for p in pin], [p + 4 * dout for p in pout]
            tail = (ref(slab_in), ref(slab)) if axis == 2 else (ref(slab),)
            if count == 1:
                f3d.check(getattr(hip, name)(a[0], b[0], ow, oh, od, n, *tail), what)
            else:
                f3d.check(getattr(hip, name + "_n")(_dev_array(a), _dev_array(b), count, ow, oh, od, n, *tail), what)
            for i in range(count):
                dev.only_box_written(pout[i], exps[i], planes, oh, ow, x0=dout, what=f"{what}, volume {i}")
            dev.unchanged(pin, what)
            if exact:
                for i in range(count):
                    got = dev.get(pout[i])[planes, :oh, dout:dout + ow]
                    box = srcs[i][:src_dims[2], :src_dims[1], :W]
                    err = sr.worst(got, sr.resample_axis(box, m, axis)[z_lo:z_hi])
                    assert err <= sr.resample_bound(n, m, float(np.abs(box).max())), (what, err)
    finally:
        dev.close()


Y_RATIOS = [(37, 5), (40, 39), (19, 19), (36, 37), (5, 37), (1, 6), (9, 1)]
Z_RATIOS = [(23, 3), (25, 24), (17, 17), (23, 25), (3, 20), (1, 5), (9, 1)]
WIDTHS = [64, 37, 66, 7, 6, 3]   # W % 4 = 0, 1, 2, 3, 2, and one below four


def test_the_widths_cover_every_tail_of_the_four_wide_kernel():
    assert {w % 4 for w in WIDTHS} == {0, 1, 2, 3} and min(WIDTHS) < 4 and any(w % 4 == 2 and w > 64 for w in WIDTHS)


@pytest.mark.parametrize("n,m", Y_RATIOS)
def test_y_pass_ratios(f3d, oracle, n, m):
    """output heights 1, 5 and heights beyond the four rows of a workgroup among them"""
    check_pass(f3d, oracle, 1, n, m, W=66, other=3, count=1, exact=True)


@pytest.mark.parametrize("n,m", Z_RATIOS)
def test_z_pass_ratios(f3d, oracle, n, m):
    check_pass(f3d, oracle, 2, n, m, W=37, other=5, count=1, exact=True)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("axis,n,m", [(1, 40, 39), (1, 5, 37), (2, 23, 3), (2, 23, 25)])
def test_y_and_z_pass_widths(f3d, oracle, axis, n, m, W):
    check_pass(f3d, oracle, axis, n, m, W=W, other=3, count=3)


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("H", [1, 5, 13])
def test_z_pass_heights_and_batches(f3d, oracle, H, count):
    check_pass(f3d, oracle, 2, 9, 23, W=70, other=H, count=count, seed=H + count)


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("n,m", [(9, 1), (37, 5), (12, 13)])
def test_y_pass_heights_and_batches(f3d, oracle, n, m, count):
    check_pass(f3d, oracle, 1, n, m, W=70, other=4, count=count, seed=count)


@pytest.mark.parametrize("n,m", [(40, 39), (5, 37), (19, 19)])
def test_y_pass_on_a_window_with_z_base(f3d, oracle, n, m):
    check_pass(f3d, oracle, 1, n, m, W=37, other=8, count=2, window=(2, 3, 6))


# n, m, (z_base of the output, z_lo, z_hi): down-sampling, two up-samplings, identity
Z_WINDOWS = [(23, 9, (1, 2, 6)), (9, 23, (5, 5, 7)), (17, 23, (9, 9, 12)), (17, 17, (4, 4, 10)), (50, 7, (0, 1, 3))]


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("n,m,window", Z_WINDOWS)
def test_z_pass_between_containers_with_different_z_base(f3d, oracle, n, m, window, count):
    """The input containers hold exactly the planes [floor(z_lo delta), min(n, ceil(z_hi delta))) and start there; the output containers
    start at a plane of their own (identity: a container that holds exactly the planes read can only start at z_lo, like the output)."""
    zb_in, top = z_source_planes(n, m, *window[1:])
    assert (zb_in != window[0]) == (n != m) and (zb_in > 0 or window[0] > 0) and top - zb_in < n
    check_pass(f3d, oracle, 2, n, m, W=37, other=5, count=count, window=window, exact=True)


@pytest.mark.parametrize("short_at", ["low", "high"])
def test_z_pass_refuses_an_input_container_one_plane_short(f3d, short_at):
    """23 -> 9, output planes [2, 6) read source planes [5, 16).  A container of 11 planes that starts at 6, or at 4, lacks one of them: the
    launcher says so before it launches anything, and the output stays poison."""
    hip = f3d.hip()
    n, m, z_lo, z_hi = 23, 9, 2, 6
    lo, hi = z_source_planes(n, m, z_lo, z_hi)
    assert (lo, hi) == (5, 16)
    zb_in = lo + 1 if short_at == "low" else lo - 1
    dev = Dev(f3d, 12, 6, hi - lo)
    try:
        rng = np.random.default_rng(2)
        pin = dev.put(rng.uniform(-1, 1, (hi - lo, 6, 12)).astype(np.float32))
        pout = dev.out()
        slab_in, slab = f3d.Slab(zb_in, zb_in, zb_in + hi - lo), f3d.Slab(1, z_lo, z_hi)
        assert refused(f3d, hip.f3d_resample_z(pin, pout, 8, 5, m, n, C.byref(slab_in), C.byref(slab)), "f3d_resample_z", "planes [5,16)",
                       "container holds")
        assert refused(f3d, hip.f3d_resample_z_n(_dev_array([pin]), _dev_array([pout]), 1, 8, 5, m, n, C.byref(slab_in), C.byref(slab)),
                       "f3d_resample_z_n", "container holds")
        ok = f3d.Slab(lo, lo, hi)
        f3d.check(hip.f3d_resample_z(pin, pout, 8, 5, m, n, C.byref(ok), C.byref(f3d.Slab(1, z_lo, z_lo))))   # an empty window: nothing
        dev.unchanged([pin, pout], "refused and empty z passes")
    finally:
        dev.close()


@pytest.mark.parametrize("axis", [1, 2])
def test_an_empty_window_returns_success_and_writes_nothing(f3d, axis):
    hip = f3d.hip()
    dev = Dev(f3d, 12, 9, 7)
    try:
        pin = [dev.put(np.random.default_rng(3).uniform(-1, 1, (7, 9, 12)).astype(np.float32)) for _ in range(2)]
        pout = [dev.out() for _ in range(2)]
        slab = f3d.Slab(1, 3, 3)
        if axis == 1:
            f3d.check(hip.f3d_resample_y(pin[0], pout[0], 8, 5, 7, 9, C.byref(slab)))
            f3d.check(hip.f3d_resample_y_n(_dev_array(pin), _dev_array(pout), 2, 8, 5, 7, 9, C.byref(slab)))
        else:
            f3d.check(hip.f3d_resample_z(pin[0], pout[0], 8, 5, 7, 7, C.byref(slab), C.byref(slab)))
            f3d.check(hip.f3d_resample_z_n(_dev_array(pin), _dev_array(pout), 2, 8, 5, 7, 7, C.byref(slab), C.byref(slab)))
        dev.unchanged(pin + pout, "an empty window")
    finally:
        dev.close()


# ---- Gaussian launchers --------------------------------------------------------------------------------------------------------------

def set_taps(f3d, taps):
    f3d.check(f3d.hip().f3d_set_conv_taps(taps.ctypes.data_as(FP), len(taps)), "f3d_set_conv_taps")


def check_rows_cols(f3d, oracle, W, H, D, R, window=None, exact=False):
    """f3d_conv_rows, f3d_conv_cols after it, and f3d_conv_rows_cols, each against the oracle's pass; window = (z_base, z_lo, z_hi)"""
    hip = f3d.hip()
    rng = np.random.default_rng(10000 + 100 * W + H + R)
    taps = sr.asym_taps(R)
    z_base, z_lo, z_hi = window or (0, 0, D)
    cw, ch, cd = W + 3, H + 2, z_hi - z_base + 1
    src = box_in_container(rng, (W, H, D), (cw, ch, D), -3, 3)
    ex = np.full_like(src, np.nan)
    oracle.conv_axis(ex, src, (W, H, D), R, taps, 0)
    exy = np.full_like(src, np.nan)
    oracle.conv_axis(exy, ex, (W, H, D), R, taps, 1)
    slab = C.byref(f3d.Slab(z_base, z_lo, z_hi)) if window else None
    planes = slice(z_lo - z_base, z_hi - z_base)
    what = f"{W} x {H} x {D}, R = {R}, window {window}"
    dev = Dev(f3d, cw, ch, cd)
    try:
        set_taps(f3d, taps)
        pin = dev.put(src[z_base:z_base + cd])
        rows, cols, both = dev.out(), dev.out(), dev.out()
        f3d.check(hip.f3d_conv_rows(rows, pin, W, H, D, R, slab))
        dev.only_box_written(rows, ex[z_lo:z_hi, :H, :W], planes, H, W, what="f3d_conv_rows " + what)
        f3d.check(hip.f3d_conv_cols(cols, rows, W, H, D, R, slab))
        dev.only_box_written(cols, exy[z_lo:z_hi, :H, :W], planes, H, W, what="f3d_conv_cols " + what)
        f3d.check(hip.f3d_conv_rows_cols(both, pin, W, H, D, R, slab))
        dev.only_box_written(both, exy[z_lo:z_hi, :H, :W], planes, H, W, what="f3d_conv_rows_cols " + what)
        assert bit_same(dev.get(both)[planes, :H, :W], dev.get(cols)[planes, :H, :W])
        dev.unchanged([pin, rows], what)
        if exact:
            box = src[:D, :H, :W]
            smax = float(np.abs(box).max())
            rows64 = sr.conv_axis(box, taps, 0)
            assert sr.worst(dev.get(rows)[planes, :H, :W], rows64[z_lo:z_hi]) <= sr.conv_bound(taps, smax)
            # the column pass reads the float32 rows: its own bound, on what it was given
            given = ex[:D, :H, :W]
            assert sr.worst(dev.get(both)[planes, :H, :W], sr.conv_axis(given, taps, 1)[z_lo:z_hi]) <= sr.conv_bound(taps, float(np.abs(given).max()))
    finally:
        dev.close()


@pytest.mark.parametrize("R", sr.RADII)
@pytest.mark.parametrize("W", [65, 130])
@pytest.mark.parametrize("H", [33, 37, 70])
def test_rows_and_columns_across_tile_seams(f3d, oracle, W, H, R):
    """k_gauss_xy tiles 64 x 32 outputs: two and three tile rows with a partial last one, two and three tile columns"""
    check_rows_cols(f3d, oracle, W, H, 2, R, exact=(W, H) == (65, 37))


@pytest.mark.parametrize("R", [6, 10, 25])
@pytest.mark.parametrize("W,H", [(4, 37), (65, 3), (4, 3), (1, 1)])
def test_rows_and_columns_on_boxes_smaller_than_the_radius(f3d, oracle, W, H, R):
    check_rows_cols(f3d, oracle, W, H, 3, R)


@pytest.mark.parametrize("R", [2, 3])
def test_rows_and_columns_on_a_single_column_of_voxels(f3d, oracle, R):
    check_rows_cols(f3d, oracle, 1, 1, 3, R)


@pytest.mark.parametrize("R", sr.RADII)
def test_rows_and_columns_on_a_window_with_z_base(f3d, oracle, R):
    check_rows_cols(f3d, oracle, 65, 37, 7, R, window=(2, 3, 5))


def z_march_chunks(W, H, planes, R):
    """the plane counts of the z-chunks f3d_conv_slices gives a window of `planes` planes (the launcher's arithmetic)"""
    tiles = math.ceil(W / 64) * math.ceil(H / 4)
    chunks = min(math.ceil(2048 / tiles), max(planes // (8 * R + 8), 1))
    zchunk = math.ceil(planes / chunks)
    return [min(zchunk, planes - z) for z in range(0, planes, zchunk)]


def check_slices(f3d, oracle, W, H, D, R, window=None, exact=False):
    """f3d_conv_slices against the oracle's z pass; window = (z_lo, z_hi): the containers then hold exactly [max(0, z_lo - R),
    min(D, z_hi + R)) and start there, otherwise the whole volume and a spare plane"""
    hip = f3d.hip()
    rng = np.random.default_rng(20000 + 100 * D + R)
    taps = sr.asym_taps(R)
    z_lo, z_hi = window or (0, D)
    z_base = max(0, z_lo - R) if window else 0
    cd = min(D, z_hi + R) - z_base if window else D + 1
    cw, ch = W + 3, H + 2
    src = box_in_container(rng, (W, H, D), (cw, ch, D), -3, 3)
    exp = np.full_like(src, np.nan)
    oracle.conv_axis(exp, src, (W, H, D), R, taps, 2)
    slab = C.byref(f3d.Slab(z_base, z_lo, z_hi)) if window else None
    planes = slice(z_lo - z_base, z_hi - z_base)
    what = f"f3d_conv_slices {W} x {H} x {D}, R = {R}, window {window}, chunks {z_march_chunks(W, H, z_hi - z_lo, R)}"
    dev = Dev(f3d, cw, ch, cd)
    try:
        set_taps(f3d, taps)
        pin, pout = dev.put(src[z_base:z_base + cd]), dev.out()
        f3d.check(hip.f3d_conv_slices(pout, pin, W, H, D, R, slab), what)
        dev.only_box_written(pout, exp[z_lo:z_hi, :H, :W], planes, H, W, what=what)
        dev.unchanged([pin], what)
        if exact:
            box = src[:D, :H, :W]
            err = sr.worst(dev.get(pout)[planes, :H, :W], sr.conv_axis(box, taps, 2)[z_lo:z_hi])
            assert err <= sr.conv_bound(taps, float(np.abs(box).max())), (what, err)
    finally:
        dev.close()


# R, D, the chunks the launcher's rule gives a thin column
Z_MARCH = [(3, 70, [35, 35]), (3, 97, [33, 33, 31]), (6, 115, [58, 57]), (2, 77, [26, 26, 25]), (1, 33, [17, 16]), (10, 177, [89, 88]),
           (25, 417, [209, 208])]


@pytest.mark.parametrize("W,H", [(5, 3), (70, 9)])
@pytest.mark.parametrize("R,D,chunks", Z_MARCH)
def test_the_z_march_across_chunk_seams(f3d, oracle, R, D, chunks, W, H):
    """k_gauss_z_reg<3>, k_gauss_z_reg<6> and k_gauss_z with its LDS ring over two and three chunks, the last one shorter"""
    assert z_march_chunks(W, H, D, R) == chunks and len(chunks) > 1
    check_slices(f3d, oracle, W, H, D, R, exact=(W, H) == (5, 3))


# R, D, (z_lo, z_hi)
Z_MARCH_WINDOWS = [(3, 80, (9, 73)), (2, 60, (7, 55)), (6, 130, (9, 121))]


@pytest.mark.parametrize("R,D,window", Z_MARCH_WINDOWS)
def test_the_z_march_on_a_window_whose_chunks_start_above_z_lo(f3d, oracle, R, D, window):
    z_lo, z_hi = window
    assert len(z_march_chunks(70, 9, z_hi - z_lo, R)) == 2 and z_lo - R > 0 and z_hi + R < D
    check_slices(f3d, oracle, 70, 9, D, R, window=window)


@pytest.mark.parametrize("R,D", [(3, 2), (6, 4), (10, 4), (25, 30), (25, 24)])
def test_the_z_march_with_fewer_planes_than_the_reach_of_the_taps(f3d, oracle, R, D):
    assert D <= 2 * R and z_march_chunks(70, 9, D, R) == [D]
    check_slices(f3d, oracle, 70, 9, D, R)
    if D > 3:
        check_slices(f3d, oracle, 5, 3, D, R, window=(1, D - 2))


@pytest.mark.parametrize("short_at", ["low", "high"])
def test_the_z_march_refuses_a_container_one_plane_short(f3d, short_at):
    """R = 3, window [9, 73) of 80 planes reads [6, 76): a container of 70 planes must start at 6"""
    hip = f3d.hip()
    R, D, z_lo, z_hi = 3, 80, 9, 73
    dev = Dev(f3d, 8, 4, z_hi - z_lo + 2 * R)
    try:
        set_taps(f3d, sr.asym_taps(R))
        pin = dev.put(np.random.default_rng(4).uniform(-1, 1, (dev.cdims[2], 4, 8)).astype(np.float32))
        pout = dev.out()
        slab = f3d.Slab(z_lo - R + (1 if short_at == "low" else -1), z_lo, z_hi)
        assert refused(f3d, hip.f3d_conv_slices(pout, pin, 5, 3, D, R, C.byref(slab)), "f3d_conv_slices", "planes [6,76)", "container holds")
        dev.unchanged([pin, pout], "a refused z march")
    finally:
        dev.close()


# ---- warp ----------------------------------------------------------------------------------------------------------------------------

SPACINGS = [(0.7, 3.0, 1.3), (2.0, 1.0, 0.7)]
# (z_base, z_lo, z_hi, z_top) of 16 planes: the containers hold [z_base, z_top), the launch warps [z_lo, z_hi)
WARP_WINDOWS = [(4, 4, 16, 16),    # z_base > 0, no plane below the window: the lowest voxels can only look up
                (2, 5, 16, 16),    # z_lo > z_base
                (0, 0, 9, 12),     # z_hi < D, three planes above the window
                (3, 6, 11, 14)]    # all of it


def check_warp(f3d, oracle, dims, h, window, seed, plant=True, into_frame_0=False):
    hip = f3d.hip()
    W, H, D = dims
    (f0, f1, u, v, w), planted, share = sr.warp_case(np.random.default_rng(seed), dims, h, window, plant=plant)
    z_base, z_lo, z_hi, z_top = window or (0, 0, D, D)
    # (sr.warp_case asserts it; once more where the device is handed the flow) no voxel of the window reads frame_1 outside the container
    assert not sr.unsafe_reads(u, v, w, h, window).any()
    exp = oracle.warp(f0, f1, u, v, w, dims, h)
    cw, ch, cd = W + 3, H + 2, z_top - z_base + (0 if window else 1)
    dev = Dev(f3d, cw, ch, cd)
    try:
        ptrs = []
        for a in (f0, f1, u, v, w):
            c = np.full((cd, ch, cw), np.nan, np.float32)
            c[:z_top - z_base, :H, :W] = a[z_base:z_top]
            ptrs.append(dev.put(c))
        out = ptrs[0] if into_frame_0 else dev.out()
        slab = C.byref(f3d.Slab(z_base, z_lo, z_hi)) if window else None
        what = f"f3d_warp {dims}, h {h}, window {window}"
        f3d.check(hip.f3d_warp(*ptrs, W, H, D, *h, out, slab), what)
        planes = slice(z_lo - z_base, z_hi - z_base)
        dev.only_box_written(out, exp[z_lo:z_hi], planes, H, W, what=what)
        dev.unchanged(ptrs[1:] if into_frame_0 else ptrs, what)
        got = dev.get(out)[planes, :H, :W]
        for z, y, x, expect in planted:
            if expect == "f0":
                assert bit_same(got[z - z_lo, y, x], f0[z, y, x]), (what, "planted voxel", z, y, x)
        err = sr.worst(got, sr.warp(f0, f1, u, v, w, h)[z_lo:z_hi])
        assert err <= sr.warp_bound(float(np.abs(f1).max())), (what, err)
    finally:
        dev.close()
    return planted, share


@pytest.mark.parametrize("h", SPACINGS)
@pytest.mark.parametrize("window", [None] + WARP_WINDOWS)
def test_warp_on_slab_windows(f3d, oracle, window, h):
    planted, share = check_warp(f3d, oracle, (13, 9, 16), h, window, seed=31)
    assert 0.2 <= share <= 0.8, f"{share:.2f} of the random voxels are interpolated: both branches need a fifth"
    assert {e for *_, e in planted} == {"f0", "in"}
    if window is None:   # every planted landing of every component
        assert len(planted) >= 3 * 8


def test_the_warp_windows_hold_the_first_and_the_last_plane_between_them():
    assert any(w[1] == 0 for w in WARP_WINDOWS) and any(w[2] == 16 for w in WARP_WINDOWS)
    assert any(w[0] > 0 for w in WARP_WINDOWS) and any(w[1] > w[0] for w in WARP_WINDOWS) and any(w[2] < 16 for w in WARP_WINDOWS)


@pytest.mark.parametrize("h", SPACINGS)
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 5, 4), (5, 1, 4), (5, 4, 1), (2, 2, 2)])
def test_warp_on_the_smallest_boxes(f3d, oracle, dims, h):
    """the launcher accepts an axis of one cell: only a flow that stays on it is inside"""
    check_warp(f3d, oracle, dims, h, None, seed=sum(dims), plant=False)


def test_warp_may_write_frame_0_and_never_frame_1(f3d, oracle):
    """include/f3d.h: a voxel reads only its own voxel of frame_0, so frame_0 may receive the result (the reference's operator allows it
    too); frame_1 is gathered from and is refused as the output, before anything is launched."""
    check_warp(f3d, oracle, (13, 9, 16), SPACINGS[0], WARP_WINDOWS[3], seed=32, into_frame_0=True)
    check_warp(f3d, oracle, (13, 9, 7), SPACINGS[1], None, seed=33, into_frame_0=True)
    hip = f3d.hip()
    dev = Dev(f3d, 8, 6, 4)
    try:
        p = [dev.put(np.random.default_rng(5).uniform(-1, 1, (4, 6, 8)).astype(np.float32)) for _ in range(5)]
        assert refused(f3d, hip.f3d_warp(*p, 8, 6, 4, 1.0, 1.0, 1.0, p[1], None), "f3d_warp", "cannot serve as output")
        dev.unchanged(p, "a refused warp")
    finally:
        dev.close()


# ---- add -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 2, 3])
def test_add_on_a_window_with_z_base(f3d, oracle, count):
    """f3d_add (one volume) and f3d_add_n in containers wider and taller than the box that start at plane 3 of 12"""
    hip = f3d.hip()
    W, H, D = 70, 9, 12
    z_base, z_lo, z_hi = 3, 5, 9
    cw, ch, cd = W + 3, H + 2, 8
    rng = np.random.default_rng(40 + count)
    a = [box_in_container(rng, (W, H, D), (cw, ch, D)) for _ in range(count)]
    b = [box_in_container(rng, (W, H, D), (cw, ch, D)) for _ in range(count)]
    dev = Dev(f3d, cw, ch, cd)
    try:
        pa = [dev.put(x[z_base:z_base + cd]) for x in a]
        pb = [dev.put(x[z_base:z_base + cd]) for x in b]
        slab = C.byref(f3d.Slab(z_base, z_lo, z_hi))
        if count == 1:
            f3d.check(hip.f3d_add(pa[0], pb[0], W, H, D, slab))
        else:
            f3d.check(hip.f3d_add_n(_dev_array(pa), _dev_array(pb), count, W, H, D, slab))
        for i in range(count):
            exp = a[i].copy()
            oracle.add(exp, b[i], (W, H, D))
            dev.only_box_written(pa[i], exp[z_lo:z_hi, :H, :W], slice(z_lo - z_base, z_hi - z_base), H, W, what=f"add, volume {i} of {count}")
        dev.unchanged(pb, "add")
    finally:
        dev.close()
