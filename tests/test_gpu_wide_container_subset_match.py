"""f3d_subset_match (include/f3d_subset_match.h) past 2 and 4 GiB of a container, built on tests/wide_container.py as
tests/test_gpu_wide_container_block_match.py is: a 24 x 12 x 20 box in the corner of a container whose planes are 256 MiB forms the
byte offsets a huge volume forms.  The nodes lie four planes apart with windows of five planes: the window of node plane 7 straddles
the 2 GiB line (plane 8), that of plane 15 the 4 GiB line, and the taps of frame 1 reach two planes further.  The records equal those
of the same data in a container of the box's own size, and the restatement of tests/subset_match_ref.py; no input is changed."""
import ctypes as C

import numpy as np
import pytest

import subset_match_cases as cases
import subset_match_ref as sm
import wide_container as wc

pytestmark = pytest.mark.gpu

DIMS = (24, 12, 20)
GRID = sm.Grid((3, 3, 3), 4, (5, 2, 4), 2)
HC, DC = 8192, 20


@pytest.fixture(scope="module")
def rig(f3d):
    free, _ = f3d.mem_info()
    if free < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free (%.1f GiB)" % (free / 2.0 ** 30))
    rigs = wc.Rigs(f3d)
    yield rigs.get(HC, DC)
    rigs.close()


def test_the_premises():
    plane = wc.PITCH * HC
    planes = sorted(set(z for _, _, z in GRID.positions()))
    windows = [(z - GRID.window, z + GRID.window) for z in planes]
    assert plane == 1 << 28
    assert any(lo * plane < 1 << 31 <= hi * plane for lo, hi in windows), "no window straddles 2 GiB"
    assert any(lo * plane < 1 << 32 <= hi * plane for lo, hi in windows), "no window straddles 4 GiB"
    assert max(hi for _, hi in windows) + 2 == DIMS[2] - 1, "the taps of the last nodes do not reach the last plane"


def match(f3d, a, b, start, records):
    fn = f3d._subset_match_entry()
    info = f3d.SubsetInfo()
    grid = f3d.SubsetGrid(*GRID.origin, GRID.step, *GRID.counts, GRID.window)
    f3d.check(fn(a, b, *DIMS, C.byref(grid), sm.AFFINE, start.ctypes.data, 20, 1e-3, 2.0, records.ctypes.data, C.byref(info)),
              "f3d_subset_match")
    return info.as_dict()


def test_subset_match_in_a_wide_container(f3d, rig):
    a, b, truth = cases.analytic_pair(DIMS, np.eye(3), (0.4, 0.3, 0.25))
    a = a + cases.noise(DIMS, 51, -2, 2)
    start = cases.starts_round(GRID, truth, 0.1, 52)
    want, want_info = sm.subset_match(a, b, GRID, sm.AFFINE, start, 20, 1e-3, 2.0)
    last = [i for i, (_, _, z) in enumerate(GRID.positions()) if z == 15]
    assert want_info["status"][sm.OUTSIDE] == 0 and (want["iterations"][last] > 0).all() and want_info["status"][sm.OK] > 0

    dense = f3d.Containers(*DIMS)
    try:
        pa, pb = dense.new(a), dense.new(b)
        dense.set_current()
        dense_records = np.zeros(GRID.nodes, sm.RECORD)
        dense_info = match(f3d, pa, pb, start, dense_records)
    finally:
        dense.free()

    rig.begin(DIMS)
    pa, pb = rig.put(a), rig.put(b)
    records = np.zeros(GRID.nodes, sm.RECORD)
    records["status"] = -9
    info = match(f3d, pa, pb, start, records)
    assert records.tobytes() == dense_records.tobytes() and info == dense_info, "the records depend on the container's geometry"
    assert records.tobytes() == want.tobytes() and info == want_info
    assert rig.unchanged(pa, a) and rig.unchanged(pb, b), "a frame was written"
