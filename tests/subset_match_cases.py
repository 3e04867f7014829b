"""The cases of the subset correlation tests, written once: tests/test_subset_match_cpu.py checks on the restatement
that every case shows what it is there for, tests/test_gpu_subset_match.py holds the kernel to the restatement on the same cases."""
import functools

import numpy as np

import subset_match_ref as sm

OUTSIDE = np.float32(1e30)   # what the padding of a container holds: a tap read from it changes every sum


# ---- textures ----------------------------------------------------------------------------------------------------------------------
# sinusoids of wavelength 8 voxels and more, as (amplitude, kx, ky, kz, phase) with k in cycles per voxel
WAVES = [(40.0, 1 / 8.0, 0.0, 0.0, 0.3), (35.0, 0.0, 1 / 9.0, 0.0, 1.1), (30.0, 0.0, 0.0, 1 / 8.5, 2.0), (25.0, 1 / 13.0, 1 / 11.0, 0.0, 0.7),
         (25.0, 0.0, 1 / 12.0, -1 / 10.0, 2.9), (20.0, 1 / 10.0, 0.0, 1 / 14.0, 4.1), (15.0, 1 / 17.0, -1 / 15.0, 1 / 16.0, 5.0)]


def texture_at(x, y, z):
    """the analytic texture at any points (binary64 arrays)"""
    value = np.full(np.broadcast(x, y, z).shape, 120.0)
    for amplitude, kx, ky, kz, phase in WAVES:
        value = value + amplitude * np.sin(2.0 * np.pi * (kx * x + ky * y + kz * z) + phase)
    return value


def coordinates(dims):
    w, h, d = dims
    z, y, x = np.meshgrid(np.arange(d, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return x, y, z


def analytic_pair(dims, matrix, translation):
    """(a, b, truth): a the texture, b the same texture moved by x -> c0 + A (x - c0) + t about the volume's middle c0, both sampled
    analytically; truth(c) -> the 12 parameters at node c"""
    A, t = np.asarray(matrix, np.float64), np.asarray(translation, np.float64)
    c0 = (np.asarray(dims, np.float64) - 1.0) / 2.0
    x, y, z = coordinates(dims)
    a = texture_at(x, y, z).astype(np.float32)
    inv = np.linalg.inv(A)
    q = np.stack([x - c0[0] - t[0], y - c0[1] - t[1], z - c0[2] - t[2]])
    src = np.tensordot(inv, q, axes=1)
    b = texture_at(src[0] + c0[0], src[1] + c0[1], src[2] + c0[2]).astype(np.float32)

    def truth(c):
        u = (A - np.eye(3)) @ (np.asarray(c, np.float64) - c0) + t
        return np.array([v for r in range(3) for v in (u[r], *(A - np.eye(3))[r])])
    return a, b, truth


def rotation_z(degrees):
    s, c = np.sin(np.radians(degrees)), np.cos(np.radians(degrees))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def noise(dims, seed, lo=0.0, hi=255.0):
    w, h, d = dims
    return np.random.default_rng(seed).uniform(lo, hi, size=(d, h, w)).astype(np.float32)


def rolled(a, shift):
    """b with b(p + shift) = a(p)"""
    return np.roll(a, (shift[2], shift[1], shift[0]), axis=(0, 1, 2))


def starts_round(grid, truth, spread, seed):
    """[nodes, 12]: the truth's translation + uniform noise of +-spread per node, gradients zero"""
    rng = np.random.default_rng(seed)
    start = np.zeros((grid.nodes, 12))
    for i, c in enumerate(grid.positions()):
        start[i, 0::4] = truth(c)[0::4] + rng.uniform(-spread, spread, 3)
    return start


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, dims, cdims, grid, model, a, b, start=None, max_iterations=20, tolerance=1e-3, reach=None):
        self.name, self.dims, self.cdims, self.grid, self.model, self.a, self.b = name, dims, cdims, grid, model, a, b
        self.start = None if start is None else np.ascontiguousarray(start, np.float64)
        self.max_iterations, self.tolerance = max_iterations, tolerance
        self.reach = float(grid.window) if reach is None else float(reach)
        assert a.shape == b.shape == dims[::-1] and a.dtype == b.dtype == np.float32

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """(records, info) of the restatement: computed once, shared, left unchanged"""
        records, info = sm.subset_match(self.a, self.b, self.grid, self.model, self.start, self.max_iterations, self.tolerance, self.reach)
        records.setflags(write=False)
        return records, info

    def statuses(self):
        return set(int(s) for s in self.expected()[0]["status"])


STATUS_DIMS = (40, 36, 33)


@functools.lru_cache(maxsize=None)
def kernel_cases():
    cases = []
    shift = (0.4, -0.3, 0.25)
    # the three widths round a wave of 64 with W = 1, 2, 3, both models, a start per node
    for width, window, model in ((63, 1, sm.TRANSLATION), (64, 2, sm.AFFINE), (65, 3, sm.AFFINE), (65, 2, sm.TRANSLATION)):
        dims = (width, 20, 18)
        a, b, truth = analytic_pair(dims, np.eye(3), shift)
        b = b + noise(dims, width, -2, 2)
        grid = sm.default_grid(dims, 9 if window == 3 else 7, window)
        cases.append(Case(f"w{width}_W{window}_{'ta'[model]}", dims, (96, 22, 19), grid, model, a, b, starts_round(grid, truth, 0.3, window)))
    # W = 8 on a volume just large enough for the window, the ring and the taps of a sub-voxel shift; 8 nodes
    dims = (25, 24, 24)
    a, b, truth = analytic_pair(dims, np.eye(3), shift)
    cases.append(Case("W8", dims, (32, 25, 24), sm.Grid((10, 10, 10), 2, (2, 2, 2), 8), sm.AFFINE, a + noise(dims, 8, -3, 3), b))
    # every status of a record but SINGULAR and LOST on one grid
    cases.append(status_case())
    # SINGULAR: a texture that varies along x only has no gradient along y and z
    dims = (30, 16, 15)
    x, _, _ = coordinates(dims)
    a = (100.0 + 50.0 * np.sin(x / 2.0)).astype(np.float32)
    cases.append(Case("singular", dims, (32, 17, 16), sm.default_grid(dims, 6, 2), sm.AFFINE, a, a.copy()))
    # LOST: a reach of 0.2 voxel and starts half a voxel from the truth; node 0 starts at the truth and stays
    dims = (40, 20, 18)
    a, b, truth = analytic_pair(dims, np.eye(3), shift)
    grid = sm.default_grid(dims, 8, 3)
    start = starts_round(grid, truth, 0.0, 0)
    start[1:, 0] += 0.5
    cases.append(Case("lost", dims, (64, 21, 19), grid, sm.TRANSLATION, a, b, start, reach=0.2))
    # max_iterations 1 on a half-voxel shift: NOT_CONVERGED after one update; and 64 with a tolerance no step gets below
    a, b, truth = analytic_pair(dims, np.eye(3), (0.5, 0.5, 0.5))
    cases.append(Case("one_iteration", dims, (64, 21, 19), grid, sm.AFFINE, a, b, max_iterations=1))
    small = sm.Grid((8, 8, 8), 12, (3, 1, 1), 1)
    cases.append(Case("64_iterations", dims, (64, 21, 19), small, sm.TRANSLATION, a, b + noise(dims, 64, -4, 4), max_iterations=64,
                      tolerance=1e-30, reach=50.0))
    # taps that reach the last voxel of each face: W = 1, nodes at 2 and n - 4, points half a voxel up: the taps span 0 .. 3 and
    # n - 4 .. n - 1.  The second half of the nodes start a voxel further out along one axis each and are OUTSIDE.
    dims = (12, 12, 12)
    a, b, truth = analytic_pair(dims, np.eye(3), (0.5, 0.5, 0.5))
    grid = sm.Grid((2, 2, 2), 6, (2, 2, 2), 1)
    start = np.zeros((8, 12))
    start[:, 0::4] = 0.5
    cases.append(Case("faces", dims, (16, 13, 12), grid, sm.TRANSLATION, a, b, start, max_iterations=1))
    beyond = start.copy()
    beyond[0, 0], beyond[1, 0], beyond[2, 4], beyond[4, 8], beyond[7, 8] = -0.01, 1.0, 1.0, 1.0, 1.0
    cases.append(Case("beyond_faces", dims, (16, 13, 12), grid, sm.TRANSLATION, a, b, beyond, max_iterations=1))
    # a start far from the node (the region of b a node reads lies elsewhere in the volume)
    dims = (48, 20, 18)
    a = texture_at(*coordinates(dims)).astype(np.float32)
    grid = sm.Grid((6, 8, 8), 10, (2, 1, 1), 2)
    start = np.zeros((2, 12))
    start[:, 0], start[:, 4] = 23.0, -2.0
    cases.append(Case("far_start", dims, (64, 21, 19), grid, sm.AFFINE, a, rolled(a, (23, -2, 0)) + noise(dims, 23, -1, 1), start))
    cases.append(exact_case())
    return cases


def status_case():
    """W = 2, step 8 over 40 x 36 x 33: 80 nodes.  Node 0: a NaN in its window of a.  1: a NaN of b among its taps.  2: a constant
    window of a.  3: a constant region of b.  4: a start that points out of the box.  5: a NaN in its start.  The others converge."""
    dims = STATUS_DIMS
    a, b, truth = analytic_pair(dims, np.eye(3), (0.4, -0.3, 0.25))
    a, b = a.copy(), b.copy()
    grid = sm.default_grid(dims, 8, 2)
    pos = grid.positions()
    start = starts_round(grid, truth, 0.2, 5)

    def box(c, r):
        return tuple(slice(c[k] - r, c[k] + r + 1) for k in (2, 1, 0))
    a[pos[0][2] + 1, pos[0][1], pos[0][0] - 2] = np.nan
    b[pos[1][2], pos[1][1] + 1, pos[1][0]] = np.nan
    a[box(pos[2], 2)] = 77.0
    b[box(pos[3], 4)] = 55.0
    start[3] = 0.0      # whole voxels: the weights are exactly (0, 1, 0, 0) however they are written, and every g_i is the constant
    start[4, 0] = 20.0
    start[5, 7] = np.nan
    return Case("statuses", dims, (64, 37, 34), grid, sm.AFFINE, a, b, start)


STATUS_NODES = {0: sm.NAN, 1: sm.NAN, 2: sm.FLAT, 3: sm.FLAT_TARGET, 4: sm.OUTSIDE, 5: sm.NO_START}


EXACT_SHIFT = (3, -2, 1)


def exact_case():
    """b is a rolled by an integer vector and every start is exactly that vector: g == f, so dp is exactly 0"""
    dims = (41, 36, 33)
    a = noise(dims, 77)
    grid = sm.Grid((8, 8, 8), 9, (3, 3, 2), 3)       # every window, moved by the shift, has its taps inside
    start = np.zeros((grid.nodes, 12))
    start[:, 0::4] = EXACT_SHIFT
    return Case("exact", dims, (64, 37, 34), grid, sm.AFFINE, a, rolled(a, EXACT_SHIFT), start)


def check_exact(records, start):
    assert (records["status"] == sm.OK).all() and (records["iterations"] == 1).all()
    assert (records["step"] == 0.0).all()
    assert records["p"].tobytes() == np.ascontiguousarray(start, np.float64).tobytes(), "p is not the start bit for bit"
    assert (np.abs(records["zncc"] - 1.0) <= 4 * np.finfo(np.float64).eps).all()


# ---- the analytic cases (relations, on the restatement) ------------------------------------------------------------------------------
ANALYTIC_DIMS = (44, 40, 38)
ANALYTIC_WINDOW = 6
STRAIN = 0.01
ANALYTIC_GRID = sm.Grid((12, 12, 12), 10, (3, 2, 2), ANALYTIC_WINDOW)


def strained_pair():
    """1 % strain (stretch along x, the same contraction along y) and 1 degree of rotation about z, plus a sub-voxel translation"""
    A = rotation_z(1.0) @ np.diag([1.0 + STRAIN, 1.0 - STRAIN, 1.0])
    return analytic_pair(ANALYTIC_DIMS, A, (0.3, -0.2, 0.25))


def translated_pair(translation=(0.37, -0.21, 0.29)):
    return analytic_pair(ANALYTIC_DIMS, np.eye(3), translation)


def errors(records, grid, truth):
    """(rms displacement error, rms gradient error) over the nodes against the truth"""
    want = np.array([truth(c) for c in grid.positions()])
    d = records["p"] - want
    return float(np.sqrt((d[:, 0::4] ** 2).sum(axis=1).mean())), float(np.sqrt((np.delete(d, [0, 4, 8], axis=1) ** 2).sum(axis=1).mean()))


# ---- the entry, the driver and the command-line tool: written once, run on the GPU (tests/test_gpu_subset_match.py) and on the
# host-memory stand-in of tests/cpu_device_subset_match (tests/test_subset_match_cpu.py, in a child interpreter) ------------------------
def check_entries(f3d):
    """f3d_subset_match behind the public function against the restatement on every kernel case: the records byte for byte, the info"""
    for case in kernel_cases():
        g = case.grid
        nodes = f3d.subset_match(case.a, case.b, grid=f3d.SubsetGrid(*g.origin, g.step, *g.counts, g.window), start=case.start,
                                 model="affine" if case.model == sm.AFFINE else "translation", max_iterations=case.max_iterations,
                                 tolerance=case.tolerance, reach=case.reach)
        records, info = case.expected()
        wrong = [i for i in range(len(records)) if nodes.records[i].tobytes() != records[i].tobytes()]
        assert not wrong, (case.name, wrong[:4], nodes.records[wrong[0]], records[wrong[0]])
        assert nodes.info == info, case.name


DRIVER = dict(step=6, window=3)
DRIVER_KW = dict(warp_levels_count=6, outer_iterations_count=4, inner_iterations_count=5)
DRIVER_BLOCK_MATCH = dict(step=6, window=3, search=7)


def refused(error, text, call):
    try:
        call()
    except error as e:
        assert text in str(e), str(e)
        return
    raise AssertionError(f"not refused: {text}")


def nearest(x, origin, step, count):
    """the node nearest to x, the lower of two equally near (OpticalFlowE::SubsetMatch)"""
    below = 0 if x <= origin else (x - origin) // step
    if below >= count - 1:
        return count - 1
    return below + 1 if ((x - origin) - below * step) * 2 > step else below


def check_driver(f3d):
    """OpticalFlow.subset_match from each start source against the same steps by hand with the package's functions: the records, the
    rows and the summaries byte for byte."""
    import warm_start_ref as ws
    f0, f1 = ws.test_pair()
    d, h, w = f0.shape
    grid = f3d.subset_grid((w, h, d), **DRIVER)
    ref = default = sm.default_grid((w, h, d), DRIVER["step"], DRIVER["window"])
    assert [getattr(grid, n) for n, _ in grid._fields_] == [*default.origin, default.step, *default.counts, default.window]
    positions = ref.positions()

    def equal(table, hand):
        assert table.records.tobytes() == hand.records.tobytes() and table.rows.tobytes() == hand.rows.tobytes()
        assert table.info == hand.info and sorted(table.summary) == sorted(hand.summary)
        for k, v in hand.summary.items():
            assert np.float64(table.summary[k]).tobytes() == np.float64(v).tobytes() if isinstance(v, float) else table.summary[k] == v, k

    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        refused(f3d.F3dError, "no frames", lambda: flow.subset_match(start="zero", **DRIVER))
        flow.upload(f0, f1)
        refused(f3d.F3dError, "BlockMatch first", lambda: flow.subset_match(start="block-match", **DRIVER))
        refused(f3d.F3dError, "no flow is held", lambda: flow.subset_match(start="flow", **DRIVER))
        # zero, before any flow is held: no comparison
        table = flow.subset_match(start="zero", model="translation", **DRIVER)
        equal(table, f3d.subset_match(f0, f1, grid=grid, model="translation"))
        assert table.summary["compared"] == 0 and np.isnan(table.summary["rms"])
        # the block-match table: the nearest node's vector, NaN where that node is neither ok nor edge
        held = flow.block_match(**DRIVER_BLOCK_MATCH)
        m = held.grid
        start = np.zeros((len(positions), 12))
        for i, (x, y, z) in enumerate(positions):
            at = (nearest(z, m.oz, m.step, m.nz) * m.ny + nearest(y, m.oy, m.step, m.ny)) * m.nx + nearest(x, m.ox, m.step, m.nx)
            start[i, 0::4] = [held.rows[n][at] for n in "uvw"]
        table = flow.subset_match(start="block-match", reach=4.5, min_zncc=0.7, **DRIVER)
        equal(table, f3d.subset_match(f0, f1, grid=grid, start=start, reach=4.5, min_zncc=0.7))
        assert table.info["status"][sm.OK] > 0
        # the flow: the start and the comparison
        flow.compute_resident(silent=True, **DRIVER_KW)
        u, v, wz = flow.download()
        at_nodes = [np.array([c[z, y, x] for x, y, z in positions], np.float32) for c in (u, v, wz)]
        table = flow.subset_match(start="flow", **DRIVER)
        equal(table, f3d.subset_match(f0, f1, grid=grid, start=at_nodes, compare=at_nodes))
        table = flow.subset_match(start="zero", max_iterations=3, tolerance=1e-2, **DRIVER)
        equal(table, f3d.subset_match(f0, f1, grid=grid, max_iterations=3, tolerance=1e-2, compare=at_nodes))
        assert table.summary["compared"] == table.summary["status"][sm.OK]
        with np.testing.assert_raises(ValueError):
            flow.subset_match(start="guess")
    finally:
        flow.destroy()


def check_cli(f3d, exe, out_dir):
    """flow3d --subset-match on one pair, from the flow, from zero and from the block-match table, and on a sequence of two pairs:
    <tag>_subset.csv and the printed line against OpticalFlow.subset_match after the same solve"""
    import csv
    import os
    import subprocess
    import warm_start_ref as ws
    f0, f1 = ws.test_pair()
    d, h, w = f0.shape
    paths = []
    for i, f in enumerate((f0, f1)):
        paths.append(os.path.join(out_dir, f"frame{i}.raw"))
        f.tofile(paths[-1])
    solve = ["--levels", "6", "--outer", "4"]
    kw = dict(warp_levels_count=6, outer_iterations_count=4)

    def run(tag, extra):
        out = subprocess.run([exe, "--dims", str(w), str(h), str(d), "--f32", "--frames", *paths, "--out", os.path.join(out_dir, tag),
                              "--silent"] + solve + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
        return out.stdout

    def check(tag, text, nodes):
        rows = list(csv.DictReader(open(os.path.join(out_dir, tag + "_subset.csv"))))
        assert len(rows) == len(nodes)
        names = ["ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz"]
        for got, want in zip(rows, nodes.rows):
            assert [int(got[c]) for c in "xyz"] == want["position"].tolist()
            assert got["status"] == sm.STATUS[want["status"]] and int(got["iterations"]) == want["iterations"]
            mine = np.array([float(got[c]) for c in ["u", "v", "w"] + names + ["diff_u", "diff_v", "diff_w"]], np.float32)
            theirs = np.array([want["u"], want["v"], want["w"], *want["grad"], *want["diff"]], np.float32)
            assert mine.tobytes() == theirs.tobytes() or (np.isnan(mine) == np.isnan(theirs)).all() and (mine[~np.isnan(mine)] == theirs[~np.isnan(theirs)]).all()
            assert np.float64(float(got["zncc"])).tobytes() == np.float64(want["zncc"]).tobytes()
        s = nodes.summary
        line = "subset match: %d nodes" % s["nodes"] + "".join(", %d %s" % (s["status"][k], sm.STATUS[k]) for k in range(10))
        line += ", median zncc %.4f, |flow - subset| over %d nodes: rms %.4f, median %.4f, p95 %.4f" % (s["median_zncc"], s["compared"], s["rms"],
                                                                                                    s["median"], s["p95"])
        assert line in text, (line, text[-800:])

    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **kw)
        text = run("flow", ["--subset-match", "--subset-step", "6", "--subset-window", "3"])
        check("flow", text, flow.subset_match(start="flow", **DRIVER))
        text = run("zero", ["--subset-match", "--subset-step", "6", "--subset-window", "3", "--subset-start", "zero", "--subset-model",
                            "translation", "--subset-iterations", "5", "--subset-tolerance", "0.01", "--subset-min-zncc", "0.9"])
        check("zero", text, flow.subset_match(start="zero", model="translation", max_iterations=5, tolerance=0.01, min_zncc=0.9, **DRIVER))
    finally:
        flow.destroy()
    # a sequence of two pairs: one table and one line per pair, each measured on that pair's frames beside that pair's flow
    f2 = ws.test_pair(shift=(9.0, -6.0, 4.5))[1]
    paths.append(os.path.join(out_dir, "frame2.raw"))
    f2.tofile(paths[-1])
    text = run("seq", ["--subset-match", "--subset-step", "6", "--subset-window", "3"])
    assert text.count("subset match: ") == 2
    for k, (a, b) in enumerate(((f0, f1), (f1, f2))):
        flow = f3d.OpticalFlow()
        flow.initialize(w, h, d)
        try:
            flow.upload(a, b)
            flow.compute_resident(silent=True, **kw)
            check(f"seq_{k}", text, flow.subset_match(start="flow", **DRIVER))
        finally:
            flow.destroy()
    del paths[-1]
    # from the block-match table, whose guess the solve also starts from
    text = run("nodes", ["--subset-match", "--subset-step", "6", "--subset-window", "3", "--subset-start", "block-match", "--block-match",
                         "--block-match-step", "6", "--block-match-window", "3", "--block-match-search", "7"])
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.block_match(**DRIVER_BLOCK_MATCH)
        flow.set_initial_from_nodes()
        flow.compute_resident(silent=True, initial="held", **kw)
        check("nodes", text, flow.subset_match(start="block-match", **DRIVER))
    finally:
        flow.destroy()
