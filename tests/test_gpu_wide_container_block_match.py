"""f3d_block_match and f3d_expand_nodes (include/f3d_block_match.h) past 2 and 4 GiB of a container, built on tests/wide_container.py
as tests/test_gpu_wide_container_analysis.py is for the entries of include/f3d.h: a 24 x 12 x 20 box in the corner of a container
whose planes are 256 MiB forms the byte offsets a huge volume forms.  The nodes lie three planes apart with windows of three planes:
the window of node plane 7 straddles the 2 GiB line (plane 8), that of plane 16 the 4 GiB line, and the regions of frame 1 reach a
plane further.  The records and the expanded fields equal those of the same data in a container of the box's own size, and the
restatements of tests/block_match_ref.py; nothing outside the box is written and no input is changed."""
import ctypes as C

import numpy as np
import pytest

import block_match_cases as cases
import block_match_ref as bm
import wide_container as wc

pytestmark = pytest.mark.gpu

DIMS = (24, 12, 20)
GRID = bm.Grid((2, 2, 1), 3, (7, 3, 6), 1, 1)
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
    planes = [z for _, _, z in GRID.positions()]
    windows = [(z - GRID.window, z + GRID.window) for z in sorted(set(planes))]
    assert plane == 1 << 28
    assert any(lo * plane < 1 << 31 <= hi * plane for lo, hi in windows), "no window straddles 2 GiB"
    assert any(lo * plane < 1 << 32 <= hi * plane for lo, hi in windows), "no window straddles 4 GiB"
    assert max(hi for _, hi in windows) * plane > 1 << 32 and max(hi for _, hi in windows) + GRID.radii[2] <= DIMS[2] - 1


def match(f3d, a, b, records):
    fn = f3d._block_match_entry()
    info = f3d.BlockMatchInfo()
    grid = f3d.BlockMatchGrid(*GRID.origin, GRID.step, *GRID.counts, GRID.window, *GRID.radii)
    f3d.check(fn(a, b, 0.0, 255.0, 256, *DIMS, C.byref(grid), None, records.ctypes.data, C.byref(info)), "f3d_block_match")
    return info.as_dict()


def expand(f3d, nodes, outs):
    fn = f3d._expand_nodes_entry()
    nz, ny, nx = nodes[0].shape
    f3d.check(fn(*[n.ctypes.data_as(C.POINTER(C.c_float)) for n in nodes], *GRID.origin, GRID.step, nx, ny, nz, *outs, *DIMS), "f3d_expand_nodes")


def test_block_match_and_expand_nodes_in_a_wide_container(f3d, rig):
    a = cases.noise(DIMS, 41)
    b = cases.rolled(a, (1, -1, 1)) + cases.noise(DIMS, 42, -6, 6)
    a[17, 5, 9] = np.nan
    nodes = [np.ascontiguousarray(cases.noise(GRID.counts, 43 + c, -9, 9)) for c in range(3)]
    nodes[1][5, 1, 3] = np.nan
    want_records, want_info = bm.block_match(a, b, 0.0, 255.0, 256, GRID)
    want_fields = bm.expand_nodes(*nodes, GRID.origin, GRID.step, DIMS)
    assert want_info["ok"] == GRID.nodes and want_info["nan"] > 0

    # the box's own container
    dense = f3d.Containers(*DIMS)
    try:
        pa, pb = dense.new(a), dense.new(b)
        outs = [dense.alloc() for _ in range(3)]
        dense.set_current()
        dense_records = np.zeros((GRID.nodes, bm.RECORD_WORDS), np.int32)
        dense_info = match(f3d, pa, pb, dense_records)
        expand(f3d, nodes, outs)
        dense_fields = [dense.download(o, DIMS) for o in outs]
    finally:
        dense.free()

    rig.begin(DIMS)
    pa, pb = rig.put(a), rig.put(b)
    pairs = [rig.out() for _ in range(3)]
    records = np.full((GRID.nodes, bm.RECORD_WORDS), -9, np.int32)
    info = match(f3d, pa, pb, records)
    expand(f3d, nodes, [p for p, _ in pairs])
    assert np.array_equal(records, dense_records) and info == dense_info, "the records depend on the container's geometry"
    assert np.array_equal(records, want_records) and info == want_info
    for pair, dense_field, want in zip(pairs, dense_fields, want_fields):
        box, clean = rig.written(pair, (0, DIMS[2]))
        assert clean, "f3d_expand_nodes wrote outside the box"
        assert wc.bit_same(box, dense_field), "the expanded field depends on the container's geometry"
        assert wc.bit_same(box, want)
    assert rig.unchanged(pa, a) and rig.unchanged(pb, b), "a frame was written"
