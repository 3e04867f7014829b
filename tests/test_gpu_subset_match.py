"""Subset correlation on the GPU: f3d_subset_match against the numpy restatement of tests/subset_match_ref.py bit for
bit (records compared as bytes, info, the containers round the box), every refusal, the exact case, and the public Python function.
The cases are those of tests/subset_match_cases.py, which tests/test_subset_match_cpu.py checks on the restatement."""
import ctypes as C

import numpy as np
import pytest

import subset_match_cases as cases
import subset_match_ref as sm

pytestmark = pytest.mark.gpu

KERNEL_CASES = cases.kernel_cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def container_of(vol, cdims, fill=cases.OUTSIDE):
    wc, hc, dc = cdims
    d, h, w = vol.shape
    c = np.full((dc, hc, wc), fill, np.float32)
    c[:d, :h, :w] = vol
    return c


def grid_of(f3d, grid):
    return f3d.SubsetGrid(*grid.origin, grid.step, *grid.counts, grid.window)


def run_entry(f3d, fn, ptrs, case, records, info):
    return fn(*ptrs, *case.dims, C.byref(grid_of(f3d, case.grid)), case.model, None if case.start is None else case.start.ctypes.data,
              case.max_iterations, case.tolerance, case.reach, records.ctypes.data, None if info is None else C.byref(info))


def differing(got, want):
    wrong = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    return (len(wrong), wrong[:4], got[wrong[0]], want[wrong[0]]) if wrong else None


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c.name for c in KERNEL_CASES])
def test_subset_match_equals_the_restatement_bit_for_bit(f3d, case):
    fn = f3d._subset_match_entry()
    expected, expected_info = case.expected()
    box = f3d.Containers(*case.cdims)
    try:
        held = [container_of(v, case.cdims) for v in (case.a, case.b)]
        ptrs = [box.new(c) for c in held]
        box.set_current()
        first = np.zeros(len(expected), sm.RECORD)
        first["status"] = -77
        info = f3d.SubsetInfo()
        f3d.check(run_entry(f3d, fn, ptrs, case, first, info), "f3d_subset_match")
        assert differing(first, expected) is None, case.name
        assert info.as_dict() == expected_info
        # the same call again, without info: the same bytes
        second = np.zeros(len(expected), sm.RECORD)
        f3d.check(run_entry(f3d, fn, ptrs, case, second, None), "f3d_subset_match")
        assert first.tobytes() == second.tobytes()
        # the frames and the padding round them are as they were
        for p, c in zip(ptrs, held):
            assert np.array_equal(bits(box.download(p, case.cdims)), bits(c)), "a frame was written"
    finally:
        box.free()


def test_subset_match_reads_no_padding(f3d):
    """a NaN in every voxel outside the box changes nothing: the faces case has taps on the last voxel of every face"""
    fn = f3d._subset_match_entry()
    for name in ("faces", "w65_W3_a"):
        case = [c for c in KERNEL_CASES if c.name == name][0]
        expected, expected_info = case.expected()
        box = f3d.Containers(*case.cdims)
        try:
            ptrs = [box.new(container_of(v, case.cdims, fill=np.float32(np.nan))) for v in (case.a, case.b)]
            box.set_current()
            got, info = np.zeros(len(expected), sm.RECORD), f3d.SubsetInfo()
            f3d.check(run_entry(f3d, fn, ptrs, case, got, info), "f3d_subset_match")
            assert got.tobytes() == expected.tobytes() and info.as_dict() == expected_info and info.nan == 0
        finally:
            box.free()


def test_the_exact_case(f3d):
    case = [c for c in KERNEL_CASES if c.name == "exact"][0]
    nodes = f3d.subset_match(case.a, case.b, grid=grid_of(f3d, case.grid), start=case.start)
    cases.check_exact(nodes.records, case.start)
    assert nodes.summary["status"][sm.OK] == case.grid.nodes
    assert np.array_equal(nodes.u, np.full(case.grid.counts[::-1], cases.EXACT_SHIFT[0], np.float32))


def test_subset_match_refuses_what_it_cannot_do(f3d):
    fn = f3d._subset_match_entry()
    dims = (40, 30, 20)
    box = f3d.Containers(*dims)
    try:
        a, b = (box.new(cases.noise(dims, s)) for s in (1, 2))
        box.set_current()
        names = ("ox", "oy", "oz", "step", "nx", "ny", "nz", "window")
        good = dict(a=a, b=b, dims=dims, grid=(4, 4, 4, 6, 6, 4, 2, 3), model=sm.AFFINE, start=None, iterations=3, tolerance=1e-3, reach=3.0,
                    records=True)
        records = np.zeros(48, sm.RECORD)
        records["status"] = -5
        untouched = records.tobytes()
        info = f3d.SubsetInfo(nodes=99)

        def call(**change):
            k = dict(good, **change)
            grid = None if k["grid"] is None else C.byref(f3d.SubsetGrid(*k["grid"]))
            return fn(k["a"], k["b"], *k["dims"], grid, k["model"], k["start"], k["iterations"], k["tolerance"], k["reach"],
                      records.ctypes.data if k["records"] else None, C.byref(info))

        def grid(**change):
            g = dict(zip(names, good["grid"]), **change)
            return dict(grid=tuple(g[n] for n in names))

        nan, inf = float("nan"), float("inf")
        bad = [dict(a=0), dict(b=0), dict(grid=None), dict(records=False), dict(model=2), dict(model=-1),
               grid(window=0), grid(window=9), grid(step=0), grid(nx=0), grid(nz=-1), grid(nx=2048, ny=2048, nz=2),
               grid(ox=3), grid(oy=3), grid(oz=3), grid(nx=7), grid(ny=5), grid(nz=4), grid(window=8),
               dict(iterations=0), dict(iterations=65), dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=nan),
               dict(reach=0.0), dict(reach=-2.0), dict(reach=nan),
               dict(dims=(0, 30, 20)), dict(dims=(41, 30, 20)), dict(dims=(40, 31, 20)), dict(dims=(40, 30, 21))]
        for change in bad:
            assert call(**change) != 0, change
            assert b"f3d_subset_match" in f3d.hip().f3d_last_error(), change
            assert records.tobytes() == untouched and info.nodes == 99, change
        assert call() == 0 and records.tobytes() != untouched and info.nodes == 48
        assert call(iterations=64, reach=inf, tolerance=inf) == 0                                      # the limits themselves
        assert call(**grid(window=8, ox=9, oy=9, oz=9, nx=1, ny=1, nz=1), dims=(19, 19, 19)) == 0
    finally:
        box.free()


def test_the_python_function_equals_restatement_and_host_table(f3d):
    case = [c for c in KERNEL_CASES if c.name == "statuses"][0]
    g = case.grid
    compare = [np.random.default_rng(k).normal(0.3, 0.2, g.nodes).astype(np.float32) for k in range(3)]
    nodes = f3d.subset_match(case.a, case.b, grid=grid_of(f3d, g), start=case.start, min_zncc=0.9, compare=compare)
    records, info = case.expected()
    rows, summary = sm.table(records, g, 0.9, compare)
    assert nodes.records.tobytes() == records.tobytes() and nodes.info == info
    assert nodes.rows.tobytes() == rows.tobytes() and same(nodes.summary, summary)
    assert nodes.u.shape == g.counts[::-1] and len(nodes.grad) == 9 and nodes.grad[4].shape == g.counts[::-1]
    assert len(nodes.as_table()) == g.nodes and nodes.as_table()[5]["status"] == "no_start"
    # the defaults: the grid subset_grid lays, zero start, the affine model
    small = [c for c in KERNEL_CASES if c.name == "W8"][0]
    nodes = f3d.subset_match(small.a, small.b, grid=f3d.subset_grid(small.dims, step=2, window=8, origin=(10, 10, 10), counts=(2, 2, 2)))
    assert nodes.records.tobytes() == small.expected()[0].tobytes()
    # node gradients feed the tensor kernels as they are
    principal = f3d.principal_from_gradient(nodes.grad, fields=("val",))
    assert principal["e1"].shape == (2, 2, 2)
    with pytest.raises(ValueError):
        f3d.subset_match(case.a, case.b[:-1])
    with pytest.raises(ValueError):
        f3d.subset_match(case.a, case.b, model="quadratic")
    with pytest.raises(ValueError):
        f3d.subset_match(case.a, case.b, grid=grid_of(f3d, g), start=np.zeros((3, 12)))
    with pytest.raises(ValueError):
        f3d.subset_grid((18, 40, 40))          # the default window of 8 and its ring need 19


def test_the_driver_equals_the_same_steps_by_hand(f3d):
    cases.check_driver(f3d)


def test_flow3d_subset_match_writes_the_table_of_the_python_calls(f3d, tmp_path):
    import os
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-flow3d_amd", "bin", "flow3d")
    cases.check_cli(f3d, exe, str(tmp_path))


def same(got, want):
    """two summaries: the same keys, the counts equal, the binary64 the same bits (NaN included)"""
    assert sorted(got) == sorted(want)
    return all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() if isinstance(want[k], float) else got[k] == want[k] for k in want)
