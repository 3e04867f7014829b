"""The weights-first launches on the MI355X (k_wpair8): f3d_solve_phi_ksi_sweep_fd -- phi / ksi of an outer iteration and its first sweep in
one launch -- and f3d_solve_sweep2_add_fd, two sweeps that store flow + increments.

Everything is bit for bit, against the oracle (phi_ksi then solve_sweep) and against the one-stage launches f3d_phi_ksi + f3d_solve_sweep,
over whole NaN-filled containers of pitch 256: inputs outside the box are NaN, outputs outside it must still be their fill.  Tile heights are
forced with F3D_PAIR8_TY, rounds of eight workgroups with F3D_PAIR8_ROUND (both read per launch).  Then the entries' refusals, and the Solve
operator with the weights-first schedule and with F3D_WEIGHTS_FIRST=0."""
import ctypes as C

import numpy as np
import pytest

from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu

H3 = (1.3, 0.9, 2.0)
ALPHA = 7.5
EPS = (0.001, 0.001)

# (W, H, D), tile height, workgroups per round (0: the default)
SHAPES = [
    ((64, 13, 4), 4, 0),       # one tile column, both x faces in one tile
    ((65, 26, 5), 8, 0),       # the halo column is the last column; one-column fold
    ((70, 11, 7), 4, 0),       # fold; odd tile rows, so band B is empty
    ((70, 21, 9), 8, 0),       # fold
    ((130, 30, 6), 12, 0),     # fold
    ((130, 52, 27), 12, 8),    # three tile classes
    ((130, 17, 22), 4, 8),     # a folded tile alone in the last class
    ((70, 21, 2), 8, 0),       # both z faces adjacent
    ((130, 30, 2), 12, 0),
]


def container_of(dims):
    W, H, D = dims
    return (256, H + 3, D + 1)


class Dev:
    def __init__(self, f3d, cdims):
        self.f3d, self.cdims = f3d, cdims
        self.cont = f3d.Containers(*cdims)
        self.cont.alloc(fill=0xFF)      # fresh containers are NaN
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


def inputs(rng, dims, cdims, zero_increments):
    mk = lambda lo, hi: box_in_container(rng, dims, cdims, lo, hi)
    arrs = [mk(0, 255), mk(0, 255), mk(-3, 3), mk(-3, 3), mk(-3, 3), mk(-0.5, 0.5), mk(-0.5, 0.5), mk(-0.5, 0.5)]
    if zero_increments:
        W, H, D = dims
        for a in arrs[5:]:
            a[:D, :H, :W] = 0
    return arrs


@pytest.fixture
def tiles(monkeypatch):
    def force(ty, per_round):
        monkeypatch.setenv("F3D_PAIR8_TY", str(ty))
        if per_round:
            monkeypatch.setenv("F3D_PAIR8_ROUND", str(per_round))
        else:
            monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    return force


FILL = 0xFFFFFFFF      # Dev allocates with fill 0xFF: every word of a fresh container


def outside_is_fill(g, dims):
    """Bitwise: the inputs outside the box are NaN as well, so a stray store there would write a NaN -- but not this one."""
    W, H, D = dims
    outside = np.ones(g.shape, bool)
    outside[:D, :H, :W] = False
    return bool((np.ascontiguousarray(g).view(np.uint32)[outside] == FILL).all())


def all_fill(g):
    return bool((np.ascontiguousarray(g).view(np.uint32) == FILL).all())


def frame_derivatives(f3d, dev, ptr, dims):
    fd = [dev.out() for _ in range(4)]
    f3d.check(f3d.hip().f3d_frame_derivatives(ptr[0], ptr[1], *dims, *H3, *fd, None))
    return fd


@pytest.mark.parametrize("zero_increments", [False, True], ids=["increments", "zero"])
@pytest.mark.parametrize("dims,ty,per_round", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_weights_then_sweep_in_one_launch(f3d, oracle, tiles, dims, ty, per_round, zero_increments):
    tiles(ty, per_round)
    W, H, D = dims
    cdims = container_of(dims)
    rng = np.random.default_rng(sum(dims) * 7 + ty + int(zero_increments))
    arrs = inputs(rng, dims, cdims, zero_increments)
    e_phi, e_ksi = oracle.phi_ksi(*arrs, dims, H3, *EPS)
    e_inc = oracle.solve_sweep(*arrs, e_phi, e_ksi, dims, H3, ALPHA)
    hip = f3d.hip()
    dev = Dev(f3d, cdims)
    try:
        ptr = [dev.put(a) for a in arrs]
        fd = frame_derivatives(f3d, dev, ptr, dims)
        phi, ksi = dev.out(), dev.out()
        outs = [dev.out() for _ in range(3)]
        f3d.check(f3d.solve_phi_ksi_sweep_fd_entry()(*fd, *ptr[2:], W, H, D, *H3, ALPHA, *EPS, phi, ksi, *outs, None))
        got = [dev.get(p) for p in [phi, ksi] + outs]
        # the one-stage launches
        phi1, ksi1 = dev.out(), dev.out()
        outs1 = [dev.out() for _ in range(3)]
        f3d.check(hip.f3d_phi_ksi(*ptr, W, H, D, *H3, *EPS, phi1, ksi1, None))
        f3d.check(hip.f3d_solve_sweep(*ptr, phi1, ksi1, W, H, D, *H3, ALPHA, *outs1, None))
        one = [dev.get(p) for p in [phi1, ksi1] + outs1]
        for name, g, o, e in zip(("phi", "ksi", "du", "dv", "dw"), got, one, [e_phi, e_ksi] + list(e_inc)):
            bad = int((g[:D, :H, :W].view(np.uint32) != e[:D, :H, :W].view(np.uint32)).sum())
            print(f"{name}: {bad} voxels differ from the oracle")
            assert bit_same(g[:D, :H, :W], e[:D, :H, :W]), f"{name}: differs from the oracle"
            assert bit_same(g[:D, :H, :W], o[:D, :H, :W]), f"{name}: differs from f3d_phi_ksi + f3d_solve_sweep"
            assert outside_is_fill(g, dims), f"{name}: written outside the box"
        for p, a in zip(ptr, arrs):
            assert bit_same(dev.get(p), a), "an input was written"
    finally:
        dev.close()


@pytest.mark.parametrize("zero_increments", [False, True], ids=["increments", "zero"])
@pytest.mark.parametrize("dims,ty,per_round", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_two_sweeps_with_the_flow_update(f3d, oracle, tiles, dims, ty, per_round, zero_increments):
    tiles(ty, per_round)
    W, H, D = dims
    cdims = container_of(dims)
    rng = np.random.default_rng(sum(dims) * 11 + ty + int(zero_increments))
    arrs = inputs(rng, dims, cdims, zero_increments)
    phi, ksi = oracle.phi_ksi(*arrs, dims, H3, *EPS)
    once = oracle.solve_sweep(*arrs, phi, ksi, dims, H3, ALPHA)
    twice = oracle.solve_sweep(*arrs[:5], *once, phi, ksi, dims, H3, ALPHA)
    expect = [a.copy() for a in arrs[2:5]]
    for s, i in zip(expect, twice):
        oracle.add(s, i, dims)
    dev = Dev(f3d, cdims)
    try:
        ptr = [dev.put(a) for a in arrs + [phi, ksi]]
        fd = frame_derivatives(f3d, dev, ptr, dims)
        sums = [dev.out() for _ in range(3)]
        f3d.check(f3d.solve_sweep2_add_fd_entry()(*fd, *ptr[2:], W, H, D, *H3, ALPHA, *sums, None))
        for name, p, e in zip("uvw", sums, expect):
            g = dev.get(p)
            assert bit_same(g[:D, :H, :W], e[:D, :H, :W]), f"{name}: differs from two sweeps, then add"
            assert outside_is_fill(g, dims), f"{name}: written outside the box"
        for p, a in zip(ptr, arrs + [phi, ksi]):
            assert bit_same(dev.get(p), a), "an input was written"
    finally:
        dev.close()


@pytest.mark.parametrize("why", ["slab", "alias", "pitch", "ymarch"])
def test_both_entries_decline_and_write_nothing(f3d, monkeypatch, why):
    for name in ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND", "F3D_PAIR8_YMARCH", "F3D_PAIR8_TIGHT"):
        monkeypatch.delenv(name, raising=False)
    dims = (70, 48, 5) if why == "ymarch" else (70, 21, 9)    # five planes, rows >= 8 x planes: the fused launches march along y
    W, H, D = dims
    cdims = (128, 24, 12) if why == "pitch" else container_of(dims)
    rng = np.random.default_rng(23)
    arrs = inputs(rng, dims, cdims, False) + [box_in_container(rng, dims, cdims, 0.1, 1), box_in_container(rng, dims, cdims, 0.1, 1)]
    hip = f3d.hip()
    dev = Dev(f3d, cdims)
    try:
        ptr = [dev.put(a) for a in arrs]
        fd_host = [box_in_container(rng, dims, cdims, -1, 1) for _ in range(4)]
        fd = [dev.put(a) for a in fd_host]
        outs = [dev.out() for _ in range(5)]     # phi, ksi, three increments
        slab = C.byref(f3d.Slab(0, 2, 7)) if why == "slab" else None
        assert bool(hip.f3d_fused_launches_march_along_y(W, H, D)) == (why == "ymarch")
        o_ps, o_add = list(outs), list(outs[2:])
        if why == "alias":
            o_ps[0] = ptr[5]       # phi_out is the increment du
            o_add[1] = ptr[3]      # sum_v is the flow v ("in place")
        assert f3d.solve_phi_ksi_sweep_fd_entry()(*fd, *ptr[2:8], W, H, D, *H3, ALPHA, *EPS, *o_ps, slab) != 0
        assert hip.f3d_last_error()
        assert f3d.solve_sweep2_add_fd_entry()(*fd, *ptr[2:], W, H, D, *H3, ALPHA, *o_add, slab) != 0
        assert hip.f3d_last_error()
        for p, a in zip(ptr + fd, arrs + fd_host):
            assert bit_same(dev.get(p), a)
        for p in outs:
            assert all_fill(dev.get(p)), "a declined launch wrote something"
    finally:
        dev.close()


@pytest.fixture(scope="module")
def operator_case(oracle):
    """inputs of the operator test (the box, without a container) and the oracle's increments, weights and sums for every (outer, K):
    computed once on the 256-pitch container; the box part is what is compared"""
    rng = np.random.default_rng(5)
    dims, cdims = (70, 21, 9), (256, 24, 12)
    W, H, D = dims
    hosts = [box_in_container(rng, dims, cdims, *r) for r in [(0, 255), (0, 255), (-2, 2), (-2, 2), (-2, 2)]]
    expect = {}
    for outer, inner in [(1, 1), (2, 2), (3, 4), (3, 5)]:
        du = np.full_like(hosts[0], np.nan)
        du[:, :, :W] = 0
        dv, dw = du.copy(), du.copy()
        for _ in range(outer):
            phi, ksi = oracle.phi_ksi(*hosts, du, dv, dw, dims, H3, *EPS)
            for _ in range(inner):
                du, dv, dw = oracle.solve_sweep(*hosts, du, dv, dw, phi, ksi, dims, H3, ALPHA)
        sums = [a.copy() for a in hosts[2:]]
        for s, i in zip(sums, (du, dv, dw)):
            oracle.add(s, i, dims)
        expect[(outer, inner)] = ([du, dv, dw], sums, [phi, ksi])
    return dims, cdims, hosts, expect


# (outer, K, container width in floats): 128 floats = 512 bytes is a pitch on which the level READS FRAME DERIVATIVES but the
# weights-first launch declines (it wants 256 floats): the level's first launch declines and the level runs the other schedule
OPERATOR_CASES = [(1, 1, 256), (2, 2, 256), (3, 4, 256), (3, 5, 256), (3, 4, 128), (3, 5, 128)]


@pytest.mark.parametrize("switch", [None, "0"], ids=["default", "F3D_WEIGHTS_FIRST=0"])
@pytest.mark.parametrize("outer,inner,width", OPERATOR_CASES)
def test_solve_operator_on_both_schedules(f3d, operator_case, monkeypatch, outer, inner, width, switch):
    """Whatever the schedule: the increments -- or, where the operator reports the flow update done, the sums --, the last outer
    iteration's weights in the caller's arrays, the flow untouched.  The update is done when the level ends in one sweep (an odd K on the
    old schedule, an even K >= 2 on the new one) or, on the new schedule, in two sweeps (an odd K >= 3).  The new schedule is taken on a
    256-float pitch with K >= 2 (one sweep per outer iteration: the level does not read frame derivatives)."""
    dims, cdims, hosts, expect = operator_case
    W, H, D = dims
    if switch is None:
        monkeypatch.delenv("F3D_WEIGHTS_FIRST", raising=False)
    else:
        monkeypatch.setenv("F3D_WEIGHTS_FIRST", switch)
    for name in ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND"):
        monkeypatch.delenv(name, raising=False)
    if width != cdims[0]:
        cdims = (width,) + cdims[1:]
        hosts = [np.ascontiguousarray(h[:, :, :width]) for h in hosts]
    cont = f3d.Containers(*cdims)
    ptrs = [cont.new(h) for h in hosts]
    names = ["dev_flow_du", "dev_flow_dv", "dev_flow_dw", "dev_phi", "dev_ksi", "dev_temp_du", "dev_temp_dv", "dev_temp_dw"]
    extra = {n: cont.new() for n in names}
    op = f3d.Operation("solve")
    assert op.initialize(cont)
    try:
        vals = op.execute(dev_frame_0=ptrs[0], dev_frame_1=ptrs[1], dev_flow_u=ptrs[2], dev_flow_v=ptrs[3], dev_flow_w=ptrs[4],
                          outer_iterations_count=outer, inner_iterations_count=inner, equation_alpha=ALPHA, equation_smoothness=EPS[0],
                          equation_data=EPS[1], hx=H3[0], hy=H3[1], hz=H3[2], data_size=dims, flow_update=False, **extra)
        f3d.sync()
        weights_first = switch is None and inner >= 2 and width % 256 == 0
        done = inner >= 2 if weights_first else inner % 2 == 1
        print(f"outer {outer}, K {inner}, width {width}, weights first {weights_first}: flow_update reported {vals['flow_update']}")
        assert vals["flow_update"] is done
        incs, sums, weights = expect[(outer, inner)]
        for c in "uvw":
            assert {vals[f"dev_flow_d{c}"], vals[f"dev_temp_d{c}"]} == {extra[f"dev_flow_d{c}"], extra[f"dev_temp_d{c}"]}
        assert vals["dev_phi"] == extra["dev_phi"] and vals["dev_ksi"] == extra["dev_ksi"]
        for key, e in zip(names[:5], (sums if done else incs) + weights):
            assert bit_same(cont.download(vals[key], cdims)[:D, :H, :W], e[:D, :H, :W]), key
        for p, a in zip(ptrs[2:], hosts[2:]):
            assert bit_same(cont.download(p, cdims), a), "the operator wrote the flow"
    finally:
        op.destroy()
        cont.free()
