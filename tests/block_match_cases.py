"""The cases of the block matching tests, shared by tests/test_block_match_cpu.py (which checks on the restatement
that every case shows what it is there for) and tests/test_gpu_search_block_match.py (which holds the kernel to the restatement)."""
import numpy as np

import block_match_ref as bm
import warm_start_ref as ws

OUTSIDE = np.float32(1e30)   # what the padding of a container holds: far above every range, so a voxel read from it changes the sums


def noise(dims, seed, lo=0.0, hi=255.0):
    w, h, d = dims
    return np.random.default_rng(seed).uniform(lo, hi, size=(d, h, w)).astype(np.float32)


def rolled(a, shift):
    """b with b(p + shift) = a(p): the flow of the pair (a, b) is `shift` = (x, y, z) wherever it stays inside"""
    return np.roll(a, (shift[2], shift[1], shift[0]), axis=(0, 1, 2))


def default_grid(dims, step, window, radii):
    """the grid block_match_grid of the package lays: as many nodes as fit, centred"""
    first, count = [], []
    for n in dims:
        room = n - 1 - 2 * window
        o = window + (room % step) // 2
        first.append(o)
        count.append((n - 1 - window - o) // step + 1)
    return bm.Grid(first, step, count, window, radii)


class Case:
    def __init__(self, name, dims, cdims, grid, a, b, bins=256, bounds=(0.0, 255.0), centre=None):
        self.name, self.dims, self.cdims, self.grid, self.a, self.b = name, dims, cdims, grid, a, b
        self.bins, self.bounds, self.centre = bins, bounds, centre
        assert a.shape == b.shape == dims[::-1]

    def expected(self):
        return bm.block_match(self.a, self.b, *self.bounds, self.bins, self.grid, self.centre)


def kernel_cases():
    cases = []
    cd = (96, 22, 19)
    # the three widths round a wave of 64, W = 1, 2, 3, step 5; every node next to a face has candidates outside the box
    for width, window, radii in ((63, 1, (2, 2, 2)), (64, 2, (3, 0, 2)), (65, 3, (2, 1, 2))):
        dims = (width, 20, 18)
        a = noise(dims, width)
        cases.append(Case(f"w{width}", dims, cd, default_grid(dims, 5, window, radii), a, rolled(a, (1, 0, -1)) + noise(dims, 1, -8, 8)))
    # radius 4, few nodes
    dims = (30, 20, 18)
    a = noise(dims, 4)
    cases.append(Case("r4", dims, (32, 21, 18), bm.Grid((6, 6, 6), 9, (3, 1, 1), 2, 4), a, rolled(a, (-3, 2, 4))))
    # the limit: W = 8, r = 8, one node
    dims = (36, 35, 34)
    a = noise(dims, 8)
    cases.append(Case("limit", dims, (40, 36, 35), bm.Grid((17, 17, 17), 1, (1, 1, 1), 8, 8), a, rolled(a, (-7, 8, 5))))
    # a constant window of a (node 0), constant regions of b (flat candidates), and a b that is constant wherever a node looks (none)
    dims = (40, 12, 11)
    a = noise(dims, 5)
    a[:7, :7, :7] = 80.0
    b = noise(dims, 6)
    b[:, :, 8:22] = 33.0
    cases.append(Case("flat", dims, (48, 13, 12), bm.Grid((3, 3, 3), 6, (6, 1, 1), 1, (2, 1, 1)), a, b))
    # NaN and values outside the range, in both frames
    dims = (33, 14, 12)
    rng = np.random.default_rng(9)
    a, b = noise(dims, 10, -60, 320), noise(dims, 11, -60, 320)
    a[rng.random(a.shape) < 0.03] = np.nan
    b[rng.random(b.shape) < 0.03] = np.nan
    a[2, 3, 4], b[5, 6, 7] = np.inf, -np.inf
    cases.append(Case("nan", dims, (64, 16, 13), default_grid(dims, 4, 2, (1, 2, 1)), a, b))
    # two codes, and a range that is not 0 .. 255
    dims = (31, 13, 12)
    a = noise(dims, 12, -1, 1)
    cases.append(Case("bins2", dims, (64, 14, 13), default_grid(dims, 4, 2, 2), a, rolled(a, (1, -1, 2)), bins=2, bounds=(-1.0, 1.0)))
    cases.append(Case("bins200", dims, (64, 14, 13), default_grid(dims, 4, 2, 2), a, rolled(a, (1, -1, 2)), bins=200, bounds=(-0.5, 0.75)))
    # exact ties: period 2 along x and 3 along y, linear along z (a constant offset does not change a ZNCC), b == a, and codes that
    # are the values themselves (256 bins over 0 .. 256): shifts by (2 i, 3 j, k) score alike, the smallest index wins
    dims = (24, 20, 9)
    z, y, x = np.meshgrid(np.arange(9), np.arange(20), np.arange(24), indexing="ij")
    a = (100.0 * (x % 2) + 40.0 * (y % 3) + 7.0 * z).astype(np.float32)
    cases.append(Case("ties", dims, (32, 21, 10), bm.Grid((8, 8, 4), 4, (3, 2, 1), 2, (4, 3, 1)), a, a.copy(), bounds=(0.0, 256.0)))
    # a search round a centre of the caller's, one triple per node, some of them pointing out of the box
    dims = (40, 30, 24)
    a = noise(dims, 13)
    grid = default_grid(dims, 7, 2, 1)
    centre = np.tile(np.array([7, -6, 5], np.int32), (grid.nodes, 1)) + np.random.default_rng(14).integers(-1, 2, (grid.nodes, 3)).astype(np.int32)
    centre[0] = (-40, 0, 0)
    cases.append(Case("centre", dims, (64, 31, 25), grid, a, rolled(a, (7, -6, 5)), centre=centre))
    return cases


# ---- exact recovery -------------------------------------------------------------------------------------------------------------
RECOVERY_DIMS, RECOVERY_SHIFT = (45, 30, 26), (3, -2, 1)
# every node reaches the shift: on a random texture one that does not can only be low
RECOVERY_GRID = dict(origin=(4, 5, 4), step=6, counts=(6, 4, 3), window=3, radii=4)


def mirrored_texture(dims, origin, step, seed):
    """A random texture that is mirror-symmetric about every node along every axis: random values on the folded coordinates
    min(t, 2 step - t), t = (x - origin) mod 2 step.  The windows one voxel below and one voxel above a node's own window then hold the
    same values in mirrored order, so the two face neighbours of an exact integer match have the same sums and the parabola's
    offset is exactly 0.  On a texture without that symmetry the two neighbours are correlations over different voxels and the offset
    of an exact match is small, not 0 (plain noise, window 3: up to 0.03)."""
    fold = []
    for n, o in zip(dims, origin):
        t = (np.arange(n) - o) % (2 * step)
        fold.append(np.minimum(t, 2 * step - t))
    values = np.random.default_rng(seed).uniform(0, 255, size=(step + 1,) * 3).astype(np.float32)
    return np.ascontiguousarray(values[fold[2][:, None, None], fold[1][None, :, None], fold[0][None, None, :]])


def recovery_case(mirrored=True):
    g = RECOVERY_GRID
    a = mirrored_texture(RECOVERY_DIMS, g["origin"], g["step"], 21) if mirrored else noise(RECOVERY_DIMS, 21)
    grid = bm.Grid(g["origin"], g["step"], g["counts"], g["window"], g["radii"])
    return Case("recovery", RECOVERY_DIMS, (64, 31, 27), grid, a, rolled(a, RECOVERY_SHIFT))


def reaches(grid, dims, shift):
    """per node: the candidates include `shift` with the target window inside the box"""
    return [all(abs(s) <= r and 0 <= p + s - grid.window and p + s + grid.window <= n - 1
                for p, s, r, n in zip(pos, shift, grid.radii, dims)) for pos in grid.positions()]


def check_recovery(rows, grid, dims=RECOVERY_DIMS, shift=RECOVERY_SHIFT, offsets=True):
    """what the issue asks of the node table of the recovery case (offsets: of the mirrored texture only, see there)"""
    hit = np.array(reaches(grid, dims, shift))
    assert hit.all() and len(hit) > 50
    assert (rows["shift"][hit] == np.array(shift)).all()
    assert (np.abs(rows["zncc"][hit] - 1.0) <= 1e-12).all()
    if offsets:
        assert (rows["offset"][hit] == 0.0).all()
        assert (rows["u"][hit] == shift[0]).all() and (rows["v"][hit] == shift[1]).all() and (rows["w"][hit] == shift[2]).all()
    else:
        # z0 is 1; the two neighbours are correlations of unrelated noise over n = 343 voxels, each about 1 / sqrt(n) = 0.054 in size,
        # and the offset is (z- - z+) / (2 (z- - 2 + z+)), about a quarter of their difference: 0.022 was seen, 0.05 is four sigma
        print("largest |offset| of an exact integer match on plain noise:", float(np.abs(rows["offset"][hit]).max()))
        assert (np.abs(rows["offset"][hit]) < 0.05).all()
    assert (rows["status"] != bm.NODE_LOW).all()


# ---- quality: DESIGN.md 28's pair, three blobs and a ripple moved by (6, -4, 3), at 14 levels ------------------------------------
QUALITY = dict(step=6, window=3, search=7)
QUALITY_LEVELS = 14
HAND_GUESS_ERROR = 1.732


def check_quality(cold, hand, guess, matched):
    """cold, hand, matched: the flows of the three solves; guess: the prepared block-match guess.  -> the four rms errors"""
    e = {"cold": ws.rms_error(cold), "hand": ws.rms_error(hand), "guess": ws.rms_error(guess), "block-match": ws.rms_error(matched)}
    print("rms error over the interior:", e)
    assert e["guess"] < HAND_GUESS_ERROR, e
    assert e["block-match"] < e["cold"] and e["block-match"] < e["hand"], e
    return e


# ---- expansion ------------------------------------------------------------------------------------------------------------------
def expand_cases():
    """name, dims, cdims, origin, step, node arrays [nz, ny, nx] x 3"""
    rng = np.random.default_rng(31)
    mk = lambda nz, ny, nx: [rng.uniform(-9, 9, size=(nz, ny, nx)).astype(np.float32) for _ in range(3)]
    cases = [(f"w{width}", (width, 20, 18), (96, 22, 19), (3, 2, 1), 5, mk(4, 4, 13)) for width in (63, 64, 65)]
    cases.append(("one_node", (20, 9, 7), (24, 10, 8), (5, 4, 3), 4, mk(1, 1, 1)))
    cases.append(("one_per_axis_x", (20, 9, 7), (24, 10, 8), (5, 1, 1), 3, mk(2, 3, 1)))
    cases.append(("one_per_axis_z", (20, 9, 7), (24, 10, 8), (2, 1, 3), 3, mk(1, 3, 6)))
    # the hull ends inside the box on both sides of every axis, and begins outside it along x
    cases.append(("hull_inside", (40, 21, 17), (64, 22, 18), (9, 6, 5), 7, mk(2, 2, 3)))
    cases.append(("origin_outside", (40, 21, 17), (64, 22, 18), (-5, 30, 2), 6, mk(3, 2, 4)))
    nodes = mk(3, 3, 4)
    nodes[0][1, 1, 2] = np.nan
    nodes[2][0, 0, 0] = np.nan
    cases.append(("nan_node", (40, 21, 17), (64, 22, 18), (4, 3, 2), 8, nodes))
    return cases


# ---- the driver and the command-line tool: written once, run on the GPU (tests/test_gpu_search_block_match.py) and on the host-memory
# stand-in of tests/cpu_device_block_match (tests/test_block_match_cpu.py, in a child interpreter) -----------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def refused(error, text, call):
    try:
        call()
    except error as e:
        assert text in str(e), str(e)
        return
    raise AssertionError(f"not refused: {text}")


DRIVER_KW = dict(warp_levels_count=6, outer_iterations_count=4, inner_iterations_count=5)


def check_driver(f3d):
    """BlockMatch + SetInitialFromNodes + the solve from the held guess against block_match, validate_displacement on the node grid,
    expand_nodes, set_initial and compute_resident(initial=) of the package: the node table, the prepared guess and the flows byte for
    byte."""
    f0, f1 = ws.test_pair()
    d, h, w = f0.shape
    kw = DRIVER_KW
    # by hand
    nodes = f3d.block_match(f0, f1, **QUALITY)
    repaired = f3d.validate_displacement(nodes.u, nodes.v, nodes.w, mode="replace", fields=("d",))
    guess = f3d.expand_nodes(repaired["u"], repaired["v"], repaired["w"], nodes.origin, nodes.step, (w, h, d))
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        hand_info = flow.set_initial(guess)
        hand_prepared = flow.initial_download()
        flow.compute_resident(silent=True, initial=guess, **kw)
        by_hand = flow.download()
        flow.initial_end()
        # the driver
        refused(f3d.F3dError, "BlockMatch first", flow.set_initial_from_nodes)
        table = flow.block_match(**QUALITY)
        assert table.rows.tobytes() == nodes.rows.tobytes() and np.array_equal(table.records, nodes.records)
        assert table.info == nodes.info and table.summary == nodes.summary
        assert (table.origin, table.step, table.counts) == (nodes.origin, nodes.step, nodes.counts)
        validated, info = flow.set_initial_from_nodes()
        assert validated == repaired["stats"] and info.as_dict() == hand_info.as_dict()
        assert same(flow.initial_download(), hand_prepared)
        flow.compute_resident(silent=True, initial="held", **kw)
        assert same(flow.download(), by_hand)
        # initial="block-match": the two calls with the defaults of block_match
        flow.compute_resident(silent=True, initial="block-match", **kw)
        short = flow.download()
        assert len(flow.block_match()) == 2 * 2 * 1
        flow.set_initial_from_nodes()
        flow.compute_resident(silent=True, initial="held", **kw)
        assert same(flow.download(), short)
        refused(f3d.F3dError, "at most 16", lambda: flow.block_match(window=3, search=14))
        refused(f3d.F3dError, "f3d_flow_block_match failed", lambda: flow.block_match(bins=1))      # the device entry refuses
        # compute() uploads its own frames after the guess is set: the two sources that read the resident pair are not its to take
        refused(ValueError, "compute_resident", lambda: flow.compute(f0, f1, silent=True, initial="block-match", **kw))
        refused(ValueError, "compute_resident", lambda: flow.compute(f0, f1, silent=True, initial="held", **kw))
    finally:
        flow.destroy()
    return nodes, repaired


def check_cli(f3d, exe, out_dir):
    """flow3d --block-match on one pair, with --block-match-only and on a sequence: the CSV against the table of the package, the flows
    against compute(initial=) from block_match_initial byte for byte, the two lines it prints"""
    import csv
    import os
    import subprocess
    f0, f1 = ws.test_pair()
    d, h, w = f0.shape
    f2 = ws.test_pair(shift=(9.0, -6.0, 4.5))[1]
    paths = []
    for i, f in enumerate((f0, f1, f2)):
        paths.append(os.path.join(out_dir, f"frame{i}.raw"))
        f.tofile(paths[-1])
    options = ["--block-match", "--block-match-step", "6", "--block-match-window", "3", "--block-match-search", "7", "--levels", "6",
               "--outer", "4"]
    kw = dict(warp_levels_count=6, outer_iterations_count=4)

    def run(tag, frames, extra):
        out = subprocess.run([exe, "--dims", str(w), str(h), str(d), "--f32", "--frames", *frames, "--out", os.path.join(out_dir, tag),
                              "--silent"] + options + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
        return out.stdout

    def expected(a, b):
        guess, nodes = f3d.block_match_initial(a, b, **QUALITY)
        flow = f3d.OpticalFlow()
        flow.initialize(w, h, d)
        try:
            return flow.compute(a, b, silent=True, initial=guess, **kw), nodes, flow.set_initial(guess)
        finally:
            flow.destroy()

    def check_table(path, nodes):
        rows = list(csv.DictReader(open(path)))
        assert len(rows) == len(nodes)
        for got, want in zip(rows, nodes.as_table()):
            assert (int(got["x"]), int(got["y"]), int(got["z"])) == (want["x"], want["y"], want["z"])
            assert tuple(int(got["shift_" + c]) for c in "xyz") == want["shift"]
            assert tuple(float(got["offset_" + c]) for c in "xyz") == want["offset"]
            assert got["status"] == want["status"] and (float(got["zncc"]) == want["zncc"] or want["zncc"] != want["zncc"])
            assert (int(got["evaluated"]), int(got["outside"]), int(got["flat"])) == (want["evaluated"], want["outside"], want["flat"])

    def written(tag, c):
        return open(os.path.join(out_dir, f"{tag}_flow-{c}-{w}-{h}-{d}.raw"), "rb").read()

    # one pair
    text = run("one", paths[:2], [])
    flow, nodes, info = expected(f0, f1)
    check_table(os.path.join(out_dir, "one_blockmatch.csv"), nodes)
    for c, e in zip("uvw", flow):
        assert written("one", c) == e.tobytes()
    s = nodes.summary
    assert f"block match: {s['nodes']} nodes, {s['ok']} ok, {s['low']} low, {s['flat']} flat, {s['edge']} edge, {s['none']} none, median shift" in text
    assert f"initial flow: {info.replaced} replaced, {info.leaving} leaving" in text and text.index("block match:") < text.index("initial flow:")
    # only the table
    text = run("only", paths[:2], ["--block-match-only"])
    check_table(os.path.join(out_dir, "only_blockmatch.csv"), nodes)
    assert "initial flow:" not in text and not os.path.exists(os.path.join(out_dir, f"only_flow-u-{w}-{h}-{d}.raw"))
    # a sequence: every pair gets its own guess
    text = run("seq", paths, [])
    assert text.count("block match:") == text.count("initial flow:") == 2
    for k, (a, b) in enumerate(((f0, f1), (f1, f2))):
        flow, nodes, _ = expected(a, b)
        check_table(os.path.join(out_dir, f"seq_{k}_blockmatch.csv"), nodes)
        for c, e in zip("uvw", flow):
            assert written(f"seq_{k}", c) == e.tobytes(), (k, c)


def check_entries(f3d, names=("w63", "flat", "nan", "bins2", "ties", "centre")):
    """the entries behind the public functions against the restatements: what the stand-in is held to (the GPU has the containers,
    the padding and every refusal looked at in tests/test_gpu_search_block_match.py)"""
    import outlier_ref
    for case in kernel_cases():
        if case.name not in names:
            continue
        g = case.grid
        nodes = f3d.block_match(case.a, case.b, step=g.step, window=g.window, search=g.radii, bins=case.bins, range=case.bounds,
                                centre=case.centre, origin=g.origin, counts=g.counts)
        records, info = case.expected()
        assert np.array_equal(nodes.records, records) and nodes.info == info, case.name
    for name, dims, _, origin, step, nodes in expand_cases():
        assert same(f3d.expand_nodes(*nodes, origin, step, dims), bm.expand_nodes(*nodes, origin, step, dims)), name
    f0, f1 = ws.test_pair()
    table = f3d.block_match(f0, f1, **QUALITY)
    got = f3d.validate_displacement(table.u, table.v, table.w, mode="replace")
    r, u, v, w, stats = outlier_ref.validate(table.u, table.v, table.w)
    assert same([got[k] for k in "ruvw"], [r, u, v, w])
    assert {k: got["stats"][k] for k in stats if k != "r_max"} == {k: v for k, v in stats.items() if k != "r_max"}
    assert np.float32(got["stats"]["r_max"]) == stats["r_max"] and stats["replaced"] > 0
