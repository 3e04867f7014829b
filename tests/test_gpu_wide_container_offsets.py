"""Every solver launch past 2 GiB (and, from the base pointer, past 4 GiB) of a container: small boxes in the corner of a container
whose planes are 256 MiB -- the byte offsets of a huge volume with 26 600 voxels of work (tests/wide_container.py).

The fused solver kernels address a z-chunk with unsigned 32-bit byte offsets from the chunk's lowest plane; only the chunk limit of the
launchers (solver_chunk_limit, csrc/f3d_pair8_plan.h) keeps them below 2^32: 7 planes here.  Each case first asserts its PREMISES from
the launcher's own arithmetic -- (a) the window has more planes than the limit, (b) a chunk forms a byte offset >= 2^31, (c) no chunk
passes the limit -- then compares bit for bit with the CPU oracle on the same box, and after every launch checks that a margin around
the box and the strip behind the view still hold the fill and that every input is unchanged.

The module sorts behind tests/test_gpu_pipeline.py, page-locks nothing and builds no host block above 0.66 MB (LABBOOK.md)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import wide_container as wc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND", "F3D_PAIR8_PLAN", "F3D_PAIR8_FOLD", "F3D_PAIR8_YMARCH", "F3D_PAIR8_TIGHT", "F3D_TRI_TY")


@pytest.fixture(scope="module")
def rigs(f3d):
    free, _ = f3d.mem_info()
    if free < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free (%.1f GiB)" % (free / 2.0 ** 30))
    r = wc.Rigs(f3d)
    yield r
    r.close()


@pytest.fixture
def switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return lambda **kw: [monkeypatch.setenv(k, str(v)) for k, v in kw.items()]


@functools.lru_cache(maxsize=None)
def _case(dims):
    from oracle import oracle as orc
    hosts = wc.solver_hosts(dims, 1000 * dims[0] + 10 * dims[1] + dims[2])
    expect = wc.solver_expectations(orc, hosts, dims)
    for a in hosts + [x for v in expect.values() for x in v]:
        a.setflags(write=False)
    return hosts, expect


def compare(res, expect, dims, what):
    for i, (got, exp) in enumerate(zip(res["boxes"], wc.expected_boxes(expect, res, dims))):
        bad = int((wc.words(got) != wc.words(exp)).sum())
        print(f"{what}: output {i}: {bad} of {got.size} words differ from the oracle")
        assert bad == 0, f"{what}: output {i} differs from the oracle in {bad} words"


# ---- the fused launches, z march: k_pair8 / k_wpair8 with the chunks F3D_PAIR8_ROUND=1 makes long ----------------------------------

def pair8_chunks(f3d, dims, window, ty, fold, limit):
    """the chunks of a k_pair8 launch, from the launcher's own plan (f3d_pair8_plan_wide reads F3D_PAIR8_ROUND and F3D_PAIR8_PLAN)"""
    W, H, D = dims
    z_lo, z_hi = window[1:] if window else (0, D)
    plan = f3d.pair8_plan_wide(W, H, z_hi - z_lo, ty, zc_limit=limit, fold=fold)
    assert plan == f3d.pair8_plan_wide(W, H, z_hi - z_lo, ty, zc_limit=limit, per_round=1, fold=fold)
    chunks = []
    for tiles, n, zc in plan.classes:
        cut = wc.uniform_chunks(z_lo, z_hi, zc)
        assert len(cut) == n and tiles > 0
        chunks += cut
    return chunks


# dims, window, tile height, fold
PAIR8_CASES = [
    ((70, 20, 19), None, 4, True),
    ((70, 20, 19), None, 4, False),
    ((70, 20, 19), None, 8, True),
    ((70, 20, 19), None, 8, False),      # F3D_PAIR8_FOLD=0: the templates with one band per tile
    ((70, 20, 28), wc.WINDOW, 4, True),
    ((70, 20, 28), wc.WINDOW, 8, True),
    ((130, 30, 19), None, 12, True),
    ((130, 30, 19), None, 12, False),    # with the rows above: every folded and unfolded instantiation at each height, k_wpair8 too
    ((130, 30, 28), wc.WINDOW, 12, True),
    ((130, 30, 28), wc.WINDOW, 12, False),
]


def _pair8_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("dims,window,ty,fold", PAIR8_CASES, ids=_pair8_id)
def test_fused_launches_march_z_past_2_gib(f3d, rigs, switches, dims, window, ty, fold):
    W, H, D = dims
    rig = rigs.get(8192, 20)
    assert rig.plane_bytes == 1 << 28
    switches(F3D_PAIR8_TY=ty, F3D_PAIR8_ROUND=1, **({} if fold else {"F3D_PAIR8_FOLD": 0}))
    limit = f3d.solver_chunk_limit(rig.plane_bytes, 2)
    assert limit == 7
    folds = fold and 1 <= W % 64 <= 32 and W > 64 and H > ty
    assert folds == fold
    chunks = pair8_chunks(f3d, dims, window, ty, folds, limit)
    offset = wc.assert_premises(chunks, 2, D, rig.plane_bytes, limit, f"k_pair8, {ty} rows")
    print(f"k_pair8 / k_wpair8, {ty} rows, window {window}: chunks {chunks}, largest offset {offset} bytes")
    if window:   # the chunk's first plane is itself past 2 GiB of the view
        assert max(wc.chunk_reach(z0, z1, 2, D)[0] - window[0] for z0, z1 in chunks) * rig.plane_bytes >= 1 << 31

    hosts, expect = _case(dims)
    case = wc.SolverCase(rig, hosts, expect["weights"], dims, window)
    compare(case.make_frame_derivatives(), expect, dims, "f3d_frame_derivatives")
    launches = [("f3d_solve_sweep2", None), ("f3d_solve_sweep2_fd", None), ("f3d_solve_sweep_phi_ksi", None),
                ("f3d_solve_sweep_phi_ksi_fd", None)]
    if window:
        launches += [(e, k) for e in ("f3d_solve_sweep_phi_ksi_edges", "f3d_solve_sweep_phi_ksi_edges_fd") for k in ((1, 1), (0, 0))]
    else:
        launches += [("f3d_solve_phi_ksi_sweep_fd", None), ("f3d_solve_sweep2_add_fd", None)]
    for name, keep in launches:
        compare(case.run(name, keep=keep), expect, dims, f"{name} keep {keep}")


# ---- streaming passes in the 256 MiB geometry: the whole 19 planes, and a window wholly above plane 16 (past 4 GiB of a view) -------

BOX = (70, 20, 19)
WINDOWS = [None, (0, 17, 19)]
WINDOW_IDS = ["whole", "above-plane-16"]


def slab_of(f3d, window):
    return C.byref(f3d.Slab(*window)) if window else None


def span_of(window, depth):
    return (window[1], window[2]) if window else (0, depth)


def wide_views(rigs, dims, window):
    rig = rigs.get(8192, 20)
    assert rig.plane_bytes == 1 << 28
    if window:
        assert window[1] * rig.plane_bytes >= 1 << 32, "the window's first plane lies past 4 GiB of its view"
    return rig, wc.Views(rig, dims)


def uniform(rng, dims, lo, hi):
    W, H, D = dims
    return rng.uniform(lo, hi, size=(D, H, W)).astype(np.float32)


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
def test_warp_past_4_gib(f3d, oracle, rigs, window):
    W, H, D = BOX
    h = (2.0, 1.0, 0.7)
    rng = np.random.default_rng(11)
    f0, f1 = uniform(rng, BOX, 0, 255), uniform(rng, BOX, 0, 255)
    u, v, w = (uniform(rng, BOX, -0.6 * n, 0.6 * n) for n in BOX)     # ~40 % of the targets leave the level
    for a, val in ((u, 2.0), (v, -1.0), (w, 0.0)):                      # exact landings
        a[::2, ::3, ::2] = val
    u[0, 0, 0] = v[D - 1, H - 1, W - 1] = np.nan
    exp = oracle.warp(f0, f1, u, v, w, BOX, h)
    rig, views = wide_views(rigs, BOX, window)
    ptr = [views.new(a) for a in (f0, f1, u, v, w)]
    out = views.new(guard=True)
    f3d.check(f3d.hip().f3d_warp(*ptr, W, H, D, *h, out, slab_of(f3d, window)))
    z0, z1 = span_of(window, D)
    views.expect(out, exp[z0:z1], z0)
    views.check("f3d_warp")


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("R", [3, 6, 10])     # the two compiled radii and a run-time one
def test_rows_and_columns_of_the_gaussian_past_4_gib(f3d, oracle, rigs, R, window):
    import stream_ref as sr
    W, H, D = BOX
    hip = f3d.hip()
    taps = sr.asym_taps(R)
    src = uniform(np.random.default_rng(100 + R), BOX, -3, 3)
    ex, exy = np.empty_like(src), np.empty_like(src)
    oracle.conv_axis(ex, src, BOX, R, taps, 0)
    oracle.conv_axis(exy, ex, BOX, R, taps, 1)
    rig, views = wide_views(rigs, BOX, window)
    f3d.check(hip.f3d_set_conv_taps(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps)))
    pin = views.new(src)
    rows, cols, both = (views.new(guard=True) for _ in range(3))
    slab, (z0, z1) = slab_of(f3d, window), span_of(window, D)
    for what, dst, frm, e in (("f3d_conv_rows", rows, pin, ex), ("f3d_conv_cols", cols, rows, exy), ("f3d_conv_rows_cols", both, pin, exy)):
        f3d.check(getattr(hip, what)(dst, frm, W, H, D, R, slab))
        views.expect(dst, e[z0:z1], z0)
        views.check(f"{what}, R = {R}")


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("R", [3, 6, 4])      # k_gauss_z_reg twice, k_gauss_z
def test_slices_of_the_gaussian_past_4_gib(f3d, oracle, rigs, R, window):
    import stream_ref as sr
    W, H, D = BOX
    taps = sr.asym_taps(R)
    src = uniform(np.random.default_rng(200 + R), BOX, -3, 3)
    ez = np.empty_like(src)
    oracle.conv_axis(ez, src, BOX, R, taps, 2)
    rig, views = wide_views(rigs, BOX, window)
    f3d.check(f3d.hip().f3d_set_conv_taps(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps)))
    pin, out = views.new(src), views.new(guard=True)
    f3d.check(f3d.hip().f3d_conv_slices(out, pin, W, H, D, R, slab_of(f3d, window)))
    z0, z1 = span_of(window, D)
    views.expect(out, ez[z0:z1], z0)
    views.check(f"f3d_conv_slices, R = {R}")


# F3D_MEDIAN_PAIR (read per call) and the window's diameter: the five 5^3 kernels, then 3^3 and 7^3
MEDIANS = [("0", 5), ("1", 5), ("2", 5), ("3", 5), (None, 5), (None, 3), (None, 7)]


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("variant,diameter", MEDIANS)
def test_median_past_4_gib(f3d, oracle, rigs, monkeypatch, variant, diameter, window):
    W, H, D = BOX
    hip = f3d.hip()
    if variant is None:
        monkeypatch.delenv("F3D_MEDIAN_PAIR", raising=False)
    else:
        monkeypatch.setenv("F3D_MEDIAN_PAIR", variant)
    rng = np.random.default_rng(300 + diameter)
    vols = [np.round(uniform(rng, BOX, -4, 4) * 2) / 2 for _ in range(3)]      # plateaus: ties everywhere
    vols = [v.astype(np.float32) for v in vols]
    exps = [oracle.median(v, BOX, diameter) for v in vols]
    rig, views = wide_views(rigs, BOX, window)
    pin = [views.new(v) for v in vols]
    one, many = views.new(guard=True), [views.new(guard=True) for _ in range(3)]
    views.by_value.update([one] + many)
    slab, (z0, z1) = slab_of(f3d, window), span_of(window, D)
    f3d.check(hip.f3d_median(pin[0], W, H, D, diameter, one, slab))
    views.expect(one, exps[0][z0:z1], z0)
    views.check(f"f3d_median {diameter}, F3D_MEDIAN_PAIR={variant}")
    f3d.check(hip.f3d_median_n(wc.dev_array(pin), 3, W, H, D, diameter, wc.dev_array(many), slab))
    for p, e in zip(many, exps):
        views.expect(p, e[z0:z1], z0)
    views.check(f"f3d_median_n {diameter}, F3D_MEDIAN_PAIR={variant}")


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
def test_add_clear_and_memset_past_4_gib(f3d, oracle, rigs, window):
    W, H, D = BOX
    hip = f3d.hip()
    rng = np.random.default_rng(400)
    a = [uniform(rng, BOX, -3, 3) for _ in range(4)]
    b = [uniform(rng, BOX, -3, 3) for _ in range(4)]
    sums = [x.copy() for x in a]
    for s, y in zip(sums, b):
        oracle.add(s, y, BOX)
    rig, views = wide_views(rigs, BOX, window)
    pa, pb = [views.new(x, guard=True) for x in a], [views.new(y) for y in b]
    slab, (z0, z1) = slab_of(f3d, window), span_of(window, D)
    f3d.check(hip.f3d_add(pa[0], pb[0], W, H, D, slab))
    views.expect(pa[0], sums[0][z0:z1], z0)
    views.check("f3d_add")
    f3d.check(hip.f3d_add_n(wc.dev_array(pa[1:]), wc.dev_array(pb[1:]), 3, W, H, D, slab))
    for p, s in zip(pa[1:], sums[1:]):
        views.expect(p, s[z0:z1], z0)
    views.check("f3d_add_n")
    f3d.check(hip.f3d_clear_box_n(wc.dev_array(pa[:3]), 3, W, H, D, slab))
    for p in pa[:3]:
        views.expect(p, np.zeros((z1 - z0, H, W), np.float32), z0)
    views.check("f3d_clear_box_n")
    # f3d_memset2d: rows 3 .. 9, columns 5 .. 34 of one plane of a view
    z, y0, x0, h, w = z1 - 1, 3, 5, 7, 30
    f3d.check(hip.f3d_memset2d(pb[0] + z * rig.plane_bytes + y0 * wc.PITCH + x0 * 4, wc.PITCH, 0x5A, w * 4, h))
    views.expect(pb[0], np.full((1, h, w), 0x5A5A5A5A, np.uint32).view(np.float32), z, y0, x0)
    views.check("f3d_memset2d")


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
def test_reductions_past_4_gib(f3d, rigs, window):
    """f3d_abs_max, f3d_flow_stats and f3d_residual_stats through the callers of tests/test_gpu_reductions.py, against numpy in binary64
    under that module's bounds: extremes exact, sums within 1e-12 of the exact sum"""
    import exact_ref as X
    import test_gpu_reductions as red
    W, H, D = BOX
    rng = np.random.default_rng(500)
    z0, z1 = span_of(window, D)
    rig, views = wide_views(rigs, BOX, window)
    sl = f3d.Slab(*window) if window else None

    def put(lo, hi):
        full = uniform(rng, BOX, lo, hi)
        full[:z0], full[z1:] = np.float32(5e4), np.float32(-6e4)      # outside the window: larger than anything inside
        return views.new(full), full[z0:z1]

    pf, f = put(-2, 2)
    assert red.abs_max(f3d, pf, BOX, sl) == X.finite_abs_max(f)
    comps = [put(-4, 4) for _ in range(3)]
    red.check_flow_stats(red.flow_stats(f3d, [p for p, _ in comps], BOX, sl), *[a for _, a in comps])
    (p0, f0), (pw, fw) = put(0, 255), put(0, 255)
    red.check_residual(red.residual_stats(f3d, p0, pw, BOX, sl), f0, fw)
    views.check("reductions")


# axis, source cells, output cells, the box's other extents (W, H, D with None on the axis); x: the row-walking kernel twice, its
# instantiation with 16 outputs and 4 pieces per lane (more than 512 cells: 700 -> 520) and the
# staged rows of k_resample_x_lds; z: a container of 20 planes resampled to 19, identity, up-sampling
RESAMPLES = [(0, 70, 61, (None, 20, 19)), (0, 37, 70, (None, 20, 19)), (0, 700, 520, (None, 4, 19)), (0, 1030, 64, (None, 4, 19)),
             (1, 20, 17, (70, None, 19)), (1, 9, 20, (70, None, 19)),
             (2, 20, 19, (70, 20, None)), (2, 19, 19, (70, 20, None)), (2, 7, 19, (70, 20, None))]


@pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("axis,n,m,rest", RESAMPLES, ids=["%s-%d-to-%d" % ("xyz"[c[0]], c[1], c[2]) for c in RESAMPLES])
def test_resampling_passes_past_4_gib(f3d, oracle, rigs, axis, n, m, rest, window):
    """f3d_resample_{x,y,z} and their _n forms; each also through pointers 4 bytes into the views, which only the generic k_resample takes"""
    hip = f3d.hip()
    src_dims = tuple(n if r is None else r for r in rest)
    dst_dims = tuple(m if r is None else r for r in rest)
    ow, oh, od = dst_dims
    name = ("f3d_resample_x", "f3d_resample_y", "f3d_resample_z")[axis]      # and f3d_resample_x_n, f3d_resample_y_n, f3d_resample_z_n
    rng = np.random.default_rng(600 + 10 * n + m)
    srcs = [uniform(rng, src_dims, -5, 5) for _ in range(3)]
    exps = []
    for s in srcs:
        e = np.empty((od, oh, ow), np.float32)
        oracle.resample_axis(s, e, dst_dims, n, axis)
        exps.append(e)
    big = tuple(max(a, b) + 1 for a, b in zip(src_dims, dst_dims))      # (one more column: the boxes also sit 4 bytes in)
    rig, views = wide_views(rigs, (big[0], big[1] - 1, 19), window)
    z0, z1 = span_of(window, od)
    slab = slab_of(f3d, window)
    tail = ((C.byref(f3d.Slab(0, 0, n)) if window else None, slab) if axis == 2 else (slab,))
    for shift in (0, 1):
        pin = [views.new(s, x0=shift) for s in srcs]
        one, many = views.new(guard=True), [views.new(guard=True) for _ in range(3)]
        f3d.check(getattr(hip, name)(pin[0] + 4 * shift, one + 4 * shift, ow, oh, od, n, *tail))
        views.expect(one, exps[0][z0:z1], z0, x0=shift)
        views.check(f"{name} {n} -> {m}, {4 * shift} bytes in")
        f3d.check(getattr(hip, name + "_n")(wc.dev_array([p + 4 * shift for p in pin]), wc.dev_array([p + 4 * shift for p in many]), 3,
                                            ow, oh, od, n, *tail))
        for p, e in zip(many, exps):
            views.expect(p, e[z0:z1], z0, x0=shift)
        views.check(f"{name}_n {n} -> {m}, {4 * shift} bytes in")


# ---- the plane movers of f3d_comm.hip, against numpy slicing, word for word; planes on either side of plane 16 -----------------------

class Staging:
    """the dense buffer of the movers: a small allocation of its own, with a host image like the views'"""

    def __init__(self, f3d, floats):
        self.f3d, self.n = f3d, floats
        self.cont = f3d.Containers(floats, 1, 1)
        self.ptr = self.cont.alloc()
        self.image = (np.arange(floats, dtype=np.uint32) | 0x7FC00000).view(np.float32)      # NaNs that tell where they came from
        self.cont.upload(self.ptr, self.image.reshape(1, 1, floats))

    def check(self, what):
        self.f3d.sync()
        got = self.cont.download(self.ptr, (self.n, 1, 1)).ravel()
        assert wc.bit_same(got, self.image), f"{what}: {int((wc.words(got) != wc.words(self.image)).sum())} words of the staging buffer differ"

    def free(self):
        self.f3d.sync()
        self.cont.free()


def ints(values):
    return (C.c_int * len(values))(*values)


def sizes(values):
    return (C.c_size_t * len(values))(*values)


def refused(f3d, status, views, staging, what):
    assert status != 0 and f3d.hip().f3d_last_error(), f"{what}: accepted"
    views.check(what + " (refused)")
    if staging is not None:
        staging.check(what + " (refused)")


@pytest.fixture
def movers(f3d, rigs):
    W, H = 70, 20
    rig, views = wide_views(rigs, (W, H, 19), None)
    rng = np.random.default_rng(700)
    fields = [uniform(rng, (W, H, 20), -9, 9) for _ in range(4)]       # all 20 planes of the container
    staging = Staging(f3d, 140_000)
    yield rig, views, fields, [views.new(a) for a in fields], staging
    staging.free()


def test_pack_and_unpack_planes_across_plane_16(f3d, movers):
    rig, views, fields, ptr, staging = movers
    hip, (W, H) = f3d.hip(), (70, 20)
    n = H * W
    f3d.check(hip.f3d_pack_planes(ptr[0], 14, 5, W, H, staging.ptr, 100))             # planes 14 .. 18: either side of plane 16
    staging.image[100:100 + 5 * n] = fields[0][14:19].ravel()
    staging.check("f3d_pack_planes")
    views.check("f3d_pack_planes")
    out = views.new(guard=True)
    f3d.check(hip.f3d_unpack_planes(out, 16, 4, W, H, staging.ptr, 100 + n))          # what was plane 15 .. 18, to planes 16 .. 19
    views.expect(out, fields[0][15:19], 16)
    views.check("f3d_unpack_planes")
    staging.check("f3d_unpack_planes")
    f3d.check(hip.f3d_pack_planes(ptr[1], 3, 0, W, H, staging.ptr, 0))                # nothing
    f3d.check(hip.f3d_unpack_planes(out, 3, 0, W, H, staging.ptr, 0))
    staging.check("zero planes")
    for what, args in (("planes outside the container", (18, 3)), ("a negative count", (4, -1)), ("a negative plane", (-1, 2))):
        refused(f3d, hip.f3d_pack_planes(ptr[0], *args, W, H, staging.ptr, 0), views, staging, "f3d_pack_planes: " + what)
        refused(f3d, hip.f3d_unpack_planes(out, *args, W, H, staging.ptr, 0), views, staging, "f3d_unpack_planes: " + what)
    refused(f3d, hip.f3d_pack_planes(ptr[0], 0, 1, 8193, H, staging.ptr, 0), views, staging, "f3d_pack_planes: wider than the container")


def segment_table(rng, n_segments, n_fields):
    """unequal counts 0 .. 3 (so the launch pads to the longest), a zero count among them, planes up to 19, dense offsets in turn"""
    count = [int(c) for c in rng.integers(0, 4, n_segments)]
    count[1], count[-1] = 0, 3
    plane0 = [int(rng.integers(0, 21 - c)) for c in count]
    plane0[0], count[0] = 15, 3       # 15 .. 17: either side of plane 16
    plane0[-1] = 17                  # 17 .. 19: the last planes of the container
    which = [i % n_fields for i in range(n_segments)]
    offset, at = [], 7
    for c in count:
        offset.append(at)
        at += c * 1400 + 3
    return which, plane0, count, offset


def test_pack_and_unpack_segments_across_plane_16(f3d, movers):
    rig, views, fields, ptr, staging = movers
    hip, (W, H) = f3d.hip(), (70, 20)
    which, plane0, count, offset = segment_table(np.random.default_rng(701), 32, 4)
    assert 0 in count and len(set(count)) > 2 and max(offset) + 3 * 1400 <= staging.n
    table = lambda ps: (wc.dev_array([ps[k] for k in which]), ints(plane0), ints(count), sizes(offset), 32, W, H, staging.ptr)
    f3d.check(hip.f3d_pack_segments(*table(ptr)))
    for k, z, c, o in zip(which, plane0, count, offset):
        staging.image[o:o + c * 1400] = fields[k][z:z + c].ravel()
    staging.check("f3d_pack_segments")
    views.check("f3d_pack_segments")
    # back into empty views at the same planes; a segment whose planes an earlier one of its view took is left out (they would race)
    outs = [views.new(guard=True) for _ in range(4)]
    taken = {k: set() for k in range(4)}
    back_plane0, back_count = [], []
    for k, z, c in zip(which, plane0, count):
        free = c > 0 and not (set(range(z, z + c)) & taken[k])
        back_count.append(c if free else 0)
        back_plane0.append(z)
        if free:
            taken[k] |= set(range(z, z + c))
    assert sum(1 for c in back_count if c) >= 8 and back_count[0] == 3 and 0 in back_count
    f3d.check(hip.f3d_unpack_segments(wc.dev_array([outs[k] for k in which]), ints(back_plane0), ints(back_count), sizes(offset), 32, W, H,
                                      staging.ptr))
    for k, z, c, o in zip(which, back_plane0, back_count, offset):
        if c:
            views.expect(outs[k], staging.image[o:o + c * 1400].reshape(c, H, W), z)
    views.check("f3d_unpack_segments")
    staging.check("f3d_unpack_segments")
    # 33 segments, a segment outside the container, a negative count: nothing is launched
    more = lambda v, x: list(v) + [x]
    t33 = (wc.dev_array([ptr[k] for k in more(which, 0)]), ints(more(plane0, 0)), ints(more(count, 1)), sizes(more(offset, 0)), 33, W, H,
           staging.ptr)
    for name in ("f3d_pack_segments", "f3d_unpack_segments"):
        refused(f3d, getattr(hip, name)(*t33), views, staging, name + ": 33 segments")
        for what, z, c in (("planes outside the container", 19, 2), ("a negative count", 2, -1)):
            bad = (wc.dev_array([ptr[k] for k in which]), ints(plane0[:-1] + [z]), ints(count[:-1] + [c]), sizes(offset), 32, W, H, staging.ptr)
            refused(f3d, getattr(hip, name)(*bad), views, staging, f"{name}: {what}")


def test_copy_planes_and_plane_segments_across_plane_16(f3d, movers):
    rig, views, fields, ptr, staging = movers
    hip, (W, H) = f3d.hip(), (70, 20)
    out = views.new(guard=True)
    f3d.check(hip.f3d_copy_planes(out, 12, ptr[0], 13, 6, W, H))       # 13 .. 18 -> 12 .. 17: both ranges on either side of plane 16
    views.expect(out, fields[0][13:19], 12)
    views.check("f3d_copy_planes between two views")
    f3d.check(hip.f3d_copy_planes(out, 18, out, 12, 2, W, H))          # within one view, disjoint planes
    views.expect(out, fields[0][13:15], 18)
    views.check("f3d_copy_planes within a view")
    f3d.check(hip.f3d_copy_planes(out, 0, ptr[1], 5, 0, W, H))         # nothing
    views.check("f3d_copy_planes of zero planes")
    # 33 triples (two launches): one destination plane each over three views, a zero count, sources from every field
    outs = [views.new(guard=True) for _ in range(3)]
    rng = np.random.default_rng(702)
    dst_k = [i % 3 for i in range(33)]
    dst_plane = [i // 3 + 9 for i in range(33)]                          # planes 9 .. 19 of each destination
    src_k = [int(k) for k in rng.integers(0, 4, 33)]
    src_plane = [int(z) for z in rng.integers(0, 20, 33)]
    count = [1] * 33
    count[5] = 0
    src_plane[32], src_plane[0] = 19, 17
    triples = lambda dk, dz, sk, sz, c: (wc.dev_array([outs[k] for k in dk]), ints(dz), wc.dev_array([ptr[k] for k in sk]), ints(sz), ints(c),
                                         len(c), W, H)
    # a triple of the SECOND launch outside the container, or with a negative count: refused before the first launch
    for what, z, c in (("planes outside the container", 20, 1), ("a negative count", 3, -1)):
        refused(f3d, hip.f3d_copy_plane_segments(*triples(dst_k, dst_plane, src_k, src_plane[:32] + [z], count[:32] + [c])), views, None,
                "f3d_copy_plane_segments: " + what)
    refused(f3d, hip.f3d_copy_planes(out, 19, ptr[0], 0, 2, W, H), views, None, "f3d_copy_planes: planes outside the container")
    refused(f3d, hip.f3d_copy_planes(out, 0, ptr[0], 0, -1, W, H), views, None, "f3d_copy_planes: a negative count")
    f3d.check(hip.f3d_copy_plane_segments(*triples(dst_k, dst_plane, src_k, src_plane, count)))
    for dk, dz, sk, sz, c in zip(dst_k, dst_plane, src_k, src_plane, count):
        if c:
            views.expect(outs[dk], fields[sk][sz:sz + 1], dz)
    views.check("f3d_copy_plane_segments, 33 triples")
    f3d.check(hip.f3d_copy_plane_segments(None, None, None, None, None, 0, W, H))
    views.check("f3d_copy_plane_segments, no triples")


# ---- the launches whose chunk only F3D_ZCHUNK sets: one child interpreter ------------------------------------------------------

def test_one_sweep_three_stage_and_k_sweep7_launches_march_z_past_2_gib(f3d, rigs, switches, tmp_path):
    """k_phiksi6, k_sweep6, k_last_sweep_flow, k_sweep7 (F3D_PAIR8=0) and k_tri at both tile heights, whole levels and a window, with
    F3D_ZCHUNK=7 in a fresh interpreter (the switch is read once per process).  launch_solver, launch_sweep2_ty and launch_tri take
    min(F3D_ZCHUNK, chunk limit) planes per chunk: restated here for the premises."""
    plane_bytes = 1 << 28
    given = {}
    for tag, dims, window, zones in wc.CHILD_CASES:
        hosts, expect = _case(dims)
        for i, a in enumerate(list(hosts) + expect["weights"]):
            given[f"{tag}/{i}"] = a
        for name, _ in wc.CHILD_LAUNCHES:
            reach = wc.SOLVER_ENTRIES[name][1]
            limit = f3d.solver_chunk_limit(plane_bytes, reach)
            assert limit == 7
            zchunk = min(7, limit)
            windows = zones if name == "f3d_phi_ksi_zones" else [window[1:] if window else (0, dims[2])]
            for z_lo, z_hi in windows:
                offset = wc.assert_premises(wc.uniform_chunks(z_lo, z_hi, zchunk), reach, dims[2], plane_bytes, limit, f"{name}, {tag}")
                print(f"{name} ({wc.CHILD_KERNELS[name]}), {tag} [{z_lo}, {z_hi}): largest offset {offset} bytes")
    inputs, results = str(tmp_path / "inputs.npz"), str(tmp_path / "results.npz")
    np.savez(inputs, **given)
    rigs.close()   # (the child makes its own allocation)
    # (the parent's environment with the switches replaced: no LD_PRELOAD is added, and one the parent runs under is not taken away)
    env = dict(os.environ, F3D_ZCHUNK="7", F3D_PAIR8="0")
    for name in SWITCHES:
        env.pop(name, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "wide_container_worker.py"), inputs, results], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
    got = np.load(results)
    for tag, dims, window, zones in wc.CHILD_CASES:
        _, expect = _case(dims)
        zs = window[1:] if window else (0, dims[2])
        for name, tri_ty in wc.CHILD_LAUNCHES:
            n = len(expect[wc.CHILD_KEYS[name]])
            res = {"key": wc.CHILD_KEYS[name], "spans": [zs] * n, "zones": zones if name == "f3d_phi_ksi_zones" else None,
                   "boxes": [got[f"{tag}/{name}/{tri_ty}/{i}"] for i in range(n)]}
            compare(res, expect, dims, f"{name} (rows {tri_ty}), {tag}")


# ---- the y march: row offsets of 426 MiB per z plane ------------------------------------------------------------------------------

YM_HC = 13653     # the largest container height (pitch 32 768) for which pair8_ymarch_rows admits D = 8: Hc * pitch * 9 < 0xf0000000


def ymarch_taken(f3d, rig, dims):
    """the launcher's rule, through its export and restated: whole level, D <= 8, (D + 1) planes below 0xf0000000 bytes"""
    taken = bool(f3d.hip().f3d_fused_launches_march_along_y(*dims))
    assert taken == (rig.plane_bytes * (dims[2] + 1) < 0xf0000000)
    return taken


@pytest.mark.parametrize("tight", [None, 0], ids=["tight", "F3D_PAIR8_TIGHT=0"])
@pytest.mark.parametrize("dims", [(70, 70, 8), (70, 40, 5), (70, 40, 4)], ids=_pair8_id)
def test_fused_launches_march_y_with_rows_426_mib_apart(f3d, rigs, switches, dims, tight):
    W, H, D = dims
    assert YM_HC * wc.PITCH * 9 < 0xf0000000 <= (YM_HC + 1) * wc.PITCH * 9
    rig = rigs.get(YM_HC + 1, 9)
    switches(F3D_PAIR8_YMARCH=1, **({} if tight is None else {"F3D_PAIR8_TIGHT": tight}))
    hosts, expect = _case(dims)
    try:
        for hc, march in ((YM_HC, True), (YM_HC + 1, D < 8)):
            rig.geometry(hc)
            assert ymarch_taken(f3d, rig, dims) == march, (hc, dims)
            if march:   # a tile's rows are z planes: the last one lies (D - 1) planes of 426.7 MiB from the first (D = 8: 2.92 GiB)
                print(f"y march, {D} planes: largest row offset {(D - 1) * rig.plane_bytes} bytes")
                assert D < 8 or (D - 1) * rig.plane_bytes >= 1 << 31
            else:       # one row more: the z march, one plane per chunk
                assert f3d.solver_chunk_limit(rig.plane_bytes, 2) == 1
            case = wc.SolverCase(rig, hosts, expect["weights"], dims, None)
            for name in ("f3d_solve_sweep2", "f3d_solve_sweep_phi_ksi"):
                compare(case.run(name), expect, dims, f"{name}, container height {hc}")
    finally:
        rig.geometry(YM_HC + 1)
