"""The weights-first launch (k_wpair8<PAIR_PS>) on tiles with ONE band, whose row waves read the x neighbours of their lanes from the
ring (stage 1, per-lane addresses: csrc/f3d_pair8_plan.h, pair8_x_neighbours) and from their own image row (stage 2, two pad columns
that the column wave fills) instead of shifting lanes.  The shapes of tests/test_gpu_weights_first.py are nearly all folded tiles; these
put the edge lanes (0 and 63: the halo piece) and the mirror lanes (x = 0, x = W - 1) of the regular tile everywhere they can be.

The harness is that file's: containers of pitch 256 filled with NaN, random inputs, tile heights forced with F3D_PAIR8_TY (read per
launch).  f3d_solve_phi_ksi_sweep_fd is compared bit for bit with the oracle (phi_ksi, then solve_sweep) and with f3d_phi_ksi +
f3d_solve_sweep; every word outside the box must still be the fill.  Then the Solve operator against F3D_WEIGHTS_FIRST=0."""
import numpy as np
import pytest

from conftest import bit_same, box_in_container
from test_gpu_weights_first import ALPHA, EPS, H3, Dev, container_of, frame_derivatives, inputs, outside_is_fill

pytestmark = pytest.mark.gpu

# (W, H, D)
SHAPES = [
    (63, 13, 4),      # W - 1 at lane 62, lane 63 outside
    (64, 14, 5),      # both faces in one tile, W - 1 at lane 63
    (33, 9, 3),       # the narrowest regular tile
    (97, 13, 4),      # right-face regular tile whose first lane is interior and whose lane 32 is W - 1
    (161, 25, 5),     # left-face, interior and right-face regular tiles
    (192, 13, 4),     # W - 1 at lane 63 of a third tile; halo pieces fetched from inside the row on both faces
    (193, 14, 3),     # interior regular tile whose right halo column is the last column of the volume, a one-column fold behind it
    (128, 26, 2),     # both z faces adjacent
]
# a tile height is run where it fits the rows: a tile row that holds rows of the volume only in its halo is never launched otherwise
CASES = [(dims, ty) for dims in SHAPES for ty in (4, 8, 12) if ty <= dims[1]]


@pytest.mark.parametrize("zero_increments", [False, True], ids=["increments", "zero"])
@pytest.mark.parametrize("dims,ty", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"ty{v}")
def test_regular_tiles_weights_then_sweep(f3d, oracle, monkeypatch, dims, ty, zero_increments):
    monkeypatch.setenv("F3D_PAIR8_TY", str(ty))
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    W, H, D = dims
    cdims = container_of(dims)
    rng = np.random.default_rng(sum(dims) * 13 + ty + int(zero_increments))
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
        phi1, ksi1 = dev.out(), dev.out()
        outs1 = [dev.out() for _ in range(3)]
        f3d.check(hip.f3d_phi_ksi(*ptr, W, H, D, *H3, *EPS, phi1, ksi1, None))
        f3d.check(hip.f3d_solve_sweep(*ptr, phi1, ksi1, W, H, D, *H3, ALPHA, *outs1, None))
        one = [dev.get(p) for p in [phi1, ksi1] + outs1]
        for name, g, o, e in zip(("phi", "ksi", "du", "dv", "dw"), got, one, [e_phi, e_ksi] + list(e_inc)):
            bad = np.argwhere(g[:D, :H, :W].view(np.uint32) != e[:D, :H, :W].view(np.uint32))
            print(f"{name}: {len(bad)} voxels differ from the oracle" + (f", columns {sorted(set(bad[:, 2].tolist()))[:12]}" if len(bad) else ""))
            assert bit_same(g[:D, :H, :W], e[:D, :H, :W]), f"{name}: differs from the oracle"
            assert bit_same(g[:D, :H, :W], o[:D, :H, :W]), f"{name}: differs from f3d_phi_ksi + f3d_solve_sweep"
            assert outside_is_fill(g, dims), f"{name}: written outside the box"
        for p, a in zip(ptr, arrs):
            assert bit_same(dev.get(p), a), "an input was written"
    finally:
        dev.close()


def test_solve_operator_on_regular_tiles_against_the_other_schedule(f3d, monkeypatch):
    """3 outer x 5 inner iterations on 161 x 25 x 5 (a left-face, an interior and a right-face regular tile): the weights-first schedule
    against F3D_WEIGHTS_FIRST=0, bit for bit -- the flow update (an odd K: done on both schedules), the weights, the flow untouched."""
    dims, cdims = (161, 25, 5), (256, 28, 6)
    W, H, D = dims
    outer, inner = 3, 5
    for name in ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND"):
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(29)
    hosts = [box_in_container(rng, dims, cdims, *r) for r in [(0, 255), (0, 255), (-2, 2), (-2, 2), (-2, 2)]]
    names = ["dev_flow_du", "dev_flow_dv", "dev_flow_dw", "dev_phi", "dev_ksi", "dev_temp_du", "dev_temp_dv", "dev_temp_dw"]
    results = {}
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("F3D_WEIGHTS_FIRST", raising=False)
        else:
            monkeypatch.setenv("F3D_WEIGHTS_FIRST", switch)
        cont = f3d.Containers(*cdims)
        ptrs = [cont.new(h) for h in hosts]
        extra = {n: cont.new() for n in names}
        op = f3d.Operation("solve")
        assert op.initialize(cont)
        try:
            vals = op.execute(dev_frame_0=ptrs[0], dev_frame_1=ptrs[1], dev_flow_u=ptrs[2], dev_flow_v=ptrs[3], dev_flow_w=ptrs[4],
                              outer_iterations_count=outer, inner_iterations_count=inner, equation_alpha=ALPHA, equation_smoothness=EPS[0],
                              equation_data=EPS[1], hx=H3[0], hy=H3[1], hz=H3[2], data_size=dims, flow_update=False, **extra)
            f3d.sync()
            assert vals["flow_update"] is True
            results[switch] = [cont.download(vals[key], cdims)[:D, :H, :W].copy() for key in names[:5]]
            for p, a in zip(ptrs[2:], hosts[2:]):
                assert bit_same(cont.download(p, cdims), a), "the operator wrote the flow"
        finally:
            op.destroy()
            cont.free()
    for key, new, old in zip(names[:5], results[None], results["0"]):
        assert np.isfinite(new).all(), key
        assert bit_same(new, old), f"{key}: the weights-first schedule differs from F3D_WEIGHTS_FIRST=0"
