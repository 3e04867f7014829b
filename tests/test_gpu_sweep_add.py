"""f3d_solve_sweep_add on the MI355X: the last sweep of a level that stores flow + new increments (k_last_sweep_flow).

Bit for bit what f3d_solve_sweep followed by f3d_add leaves in the flow, and what the oracle's solve_sweep + add give; boxes in the
corner of NaN-poisoned containers.  Then the Solve operator asked for the flow update through its bag, and one whole pyramid."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (W,H,D) box, (Wc,Hc,Dc) container: tile-column seams (70 = 64 + 6), a width of 64 k + 1, a depth below the march's ring of 4 planes
CASES = [
    ((70, 9, 20), (128, 12, 20)),
    ((65, 13, 7), (128, 16, 8)),
    ((64, 12, 3), (64, 12, 3)),
]
H3 = (1.3, 0.9, 2.0)
ALPHA = 7.5


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


def inputs(rng, dims, cdims):
    mk = lambda lo, hi: box_in_container(rng, dims, cdims, lo, hi)
    return [mk(0, 255), mk(0, 255), mk(-3, 3), mk(-3, 3), mk(-3, 3), mk(-0.5, 0.5), mk(-0.5, 0.5), mk(-0.5, 0.5)]


def oracle_sums(oracle, arrs, phi, ksi, dims, g=None):
    """solve_sweep, then add: the flow the reference's driver holds after its `flow += increments`"""
    incs = oracle.solve_sweep(*arrs, phi, ksi, dims, H3, ALPHA, g=g)
    sums = [a.copy() for a in arrs[2:5]]
    for s, i in zip(sums, incs):
        oracle.add(s, i, dims, g=g)
    return sums


@pytest.mark.parametrize("dims,cdims", CASES)
def test_sweep_add_equals_sweep_then_add(f3d, oracle, dims, cdims):
    rng = np.random.default_rng(hash(dims) % 2**32)
    W, H, D = dims
    arrs = inputs(rng, dims, cdims)
    phi, ksi = oracle.phi_ksi(*arrs, dims, H3, 0.001, 0.001)
    expect = oracle_sums(oracle, arrs, phi, ksi, dims)
    hip = f3d.hip()
    dev = Dev(f3d, cdims)
    try:
        ptr = [dev.put(a) for a in arrs + [phi, ksi]]
        sums = [dev.out() for _ in range(3)]
        f3d.check(f3d.solve_sweep_add_entry()(*ptr, W, H, D, *H3, ALPHA, *sums, None))
        got = [dev.get(p) for p in sums]
        # the route it replaces: the sweep into containers of its own, then the add into (copies of) the flow
        incs = [dev.out() for _ in range(3)]
        f3d.check(hip.f3d_solve_sweep(*ptr, W, H, D, *H3, ALPHA, *incs, None))
        flows = [dev.put(a) for a in arrs[2:5]]
        for p, q in zip(flows, incs):
            f3d.check(hip.f3d_add(p, q, W, H, D, None))
        for c, g, p, e in zip("uvw", got, flows, expect):
            assert bit_same(g[:D, :H, :W], dev.get(p)[:D, :H, :W]), f"{c}: differs from f3d_solve_sweep + f3d_add"
            assert bit_same(g[:D, :H, :W], e[:D, :H, :W]), f"{c}: differs from the oracle's solve_sweep + add"
            outside = np.ones(g.shape, bool)
            outside[:D, :H, :W] = False
            assert np.isnan(g[outside]).all(), f"{c}: written outside the box"
        # the inputs are not written
        for p, a in zip(ptr, arrs + [phi, ksi]):
            assert bit_same(dev.get(p), a)
    finally:
        dev.close()


def test_sweep_add_under_a_slab_window(f3d, oracle):
    """a window with z_lo > 0 in a container that starts BEFORE the volume (z_base < 0, rank 0 of a z-slab run)"""
    dims, cw, ch = (70, 9, 20), 128, 12
    W, H, D = dims
    rng = np.random.default_rng(17)
    arrs = inputs(rng, dims, (cw, ch, D))
    phi, ksi = oracle.phi_ksi(*arrs, dims, H3, 0.001, 0.001)
    expect = oracle_sums(oracle, arrs, phi, ksi, dims)
    z_base, z_lo, z_hi, planes = -2, 3, 11, 16          # the container holds volume planes 0 .. 13 at its planes 2 .. 15
    held = planes + z_base

    def sub(a):
        c = np.full((planes, ch, cw), np.nan, np.float32)
        c[-z_base:] = a[:held]
        return c

    dev = Dev(f3d, (cw, ch, planes))
    try:
        ptr = [dev.put(sub(a)) for a in arrs + [phi, ksi]]
        sums = [dev.out() for _ in range(3)]
        slab = f3d.Slab(z_base, z_lo, z_hi)
        f3d.check(f3d.solve_sweep_add_entry()(*ptr, W, H, D, *H3, ALPHA, *sums, C.byref(slab)))
        for c, p, e in zip("uvw", sums, expect):
            g = dev.get(p)
            assert bit_same(g[z_lo - z_base:z_hi - z_base, :H, :W], e[z_lo:z_hi, :H, :W]), c
            untouched = np.ones(g.shape, bool)
            untouched[z_lo - z_base:z_hi - z_base, :H, :W] = False
            assert np.isnan(g[untouched]).all(), f"{c}: written outside the window"
    finally:
        dev.close()


def test_sweep_add_refuses_an_output_that_is_an_input(f3d):
    dims = cdims = (64, 12, 3)
    W, H, D = dims
    rng = np.random.default_rng(3)
    arrs = inputs(rng, dims, cdims) + [box_in_container(rng, dims, cdims, 0.1, 1), box_in_container(rng, dims, cdims, 0.1, 1)]
    hip = f3d.hip()
    dev = Dev(f3d, cdims)
    try:
        ptr = [dev.put(a) for a in arrs]
        outs = [dev.out() for _ in range(3)]
        for k in (2, 5, 8):        # the flow itself ("in place"), an increment, a weight
            for slot in range(3):
                bad = list(outs)
                bad[slot] = ptr[k]
                assert f3d.solve_sweep_add_entry()(*ptr, W, H, D, *H3, ALPHA, *bad, None) != 0
                assert b"also an input" in hip.f3d_last_error()
        # nothing was launched: inputs and outputs are what they were
        for p, a in zip(ptr, arrs):
            assert bit_same(dev.get(p), a)
        for p in outs:
            assert np.isnan(dev.get(p)).all()
    finally:
        dev.close()


@pytest.mark.parametrize("inner,done", [(5, True), (4, False)])
def test_solve_operator_asked_for_the_flow_update(f3d, oracle, inner, done):
    """5 sweeps per outer iteration end in a launch of one sweep: the update is done, the sums are in the containers the bag hands back as
    dev_flow_d*.  4 sweeps end in a pair: reported not done, the increments as always."""
    rng = np.random.default_rng(5)
    dims, cdims = (70, 21, 9), (128, 24, 12)
    W, H, D = dims
    cont = f3d.Containers(*cdims)

    def put(lo, hi):
        c = box_in_container(rng, dims, cdims, lo, hi)
        return c, cont.new(c)

    hosts, ptrs = zip(*[put(*r) for r in [(0, 255), (0, 255), (-2, 2), (-2, 2), (-2, 2)]])
    names = ["dev_flow_du", "dev_flow_dv", "dev_flow_dw", "dev_phi", "dev_ksi", "dev_temp_du", "dev_temp_dv", "dev_temp_dw"]
    extra = {n: cont.new() for n in names}
    op = f3d.Operation("solve")
    assert op.initialize(cont)
    outer = 3
    try:
        vals = op.execute(dev_frame_0=ptrs[0], dev_frame_1=ptrs[1], dev_flow_u=ptrs[2], dev_flow_v=ptrs[3], dev_flow_w=ptrs[4],
                          outer_iterations_count=outer, inner_iterations_count=inner, equation_alpha=ALPHA, equation_smoothness=0.001,
                          equation_data=0.001, hx=H3[0], hy=H3[1], hz=H3[2], data_size=dims, flow_update=False, **extra)
        f3d.sync()
        assert vals["flow_update"] is done
        du = np.full_like(hosts[0], np.nan); du[:, :, :W] = 0
        dv, dw = du.copy(), du.copy()
        for _ in range(outer):
            phi, ksi = oracle.phi_ksi(*hosts, du, dv, dw, dims, H3, 0.001, 0.001)
            for _ in range(inner):
                du, dv, dw = oracle.solve_sweep(*hosts, du, dv, dw, phi, ksi, dims, H3, ALPHA)
        expect = [du, dv, dw]
        if done:
            expect = [a.copy() for a in hosts[2:]]
            for s, i in zip(expect, (du, dv, dw)):
                oracle.add(s, i, dims)
        for c in "uvw":
            assert {vals[f"dev_flow_d{c}"], vals[f"dev_temp_d{c}"]} == {extra[f"dev_flow_d{c}"], extra[f"dev_temp_d{c}"]}
        for key, e in zip(names[:5], expect + [phi, ksi]):
            assert bit_same(cont.download(vals[key], cdims)[:D, :H, :W], e[:D, :H, :W]), key
        for p, a in zip(ptrs[2:], hosts[2:]):
            assert bit_same(cont.download(p, cdims), a), "the operator wrote the flow"
    finally:
        op.destroy()
        cont.free()


def test_whole_pyramid_with_the_update_inside_the_solve_has_the_c2_digest(f3d):
    """BASELINE config 2 (the 128^3 golden pair, full default pyramid) through the resident driver, which now asks every level's solve
    for the flow update: the committed digest."""
    e = np.load(os.path.join(GOLD, "expected_oracle.npz"))
    i128 = np.load(os.path.join(GOLD, "inputs_128.npz"))
    f0, f1 = i128["frame_0"].astype(np.float32), i128["frame_1"].astype(np.float32)
    flow = f3d.OpticalFlow()
    flow.initialize(128, 128, 128)
    try:
        got = flow.compute(f0, f1, silent=True)
    finally:
        flow.destroy()
    h = hashlib.sha256()
    for v in got:
        h.update(np.ascontiguousarray(v + np.float32(0.0)).tobytes())
    assert h.hexdigest() == str(e["c2_sha256"])
