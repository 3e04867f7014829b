"""Strain over a strain window on the GPU: f3d_window_strain against its numpy restatement (tests/window_strain_ref.py) bit for bit
with its statistics, in NaN-poisoned containers larger than the box; the field selection and the refusals of the entry; the driver's
OpticalFlow.window_strain of a solved flow against window_strain() of the downloaded flow; and bin/flow3d --window-strain against the
binding.

Shapes: the kernel's tile is 32 x 8 voxels of a plane and a run is 32 planes, so the list holds widths and heights at the tile's edge
and one off, depths of a run -r and +r planes and of three runs and a remainder, next to the shapes every derived field is tried on."""
import os
import re
import subprocess

import numpy as np
import pytest

from window_strain_ref import GROUP_OF, NAMES, default_min_count, same_bits, window_strain_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
SENTINEL = 0x7F      # byte fill of the outputs: 0x7F7F7F7F = 3.39e38
RADII = (1, 2, 3)
ALL = 15
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 1, 1), (64, 64, 1), (37, 23, 11), (584, 388, 5), (31, 5, 3), (32, 5, 3), (33, 5, 3), (9, 7, 3),
          (9, 8, 3), (9, 9, 3), (7, 5, "run-r"), (7, 5, "run+r"), (7, 5, 101)]


def displacement(rng, w, h, d, r):
    """a smooth displacement plus noise; 3 % scattered NaN in one component, a NaN block, and a slab of r NaN planes next to the first
    plane of the longest axis, so that the windows of that first plane hold one plane of points only (coplanar: thin)"""
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    comps = []
    for c in range(3):
        a = (0.8 * np.sin(0.11 * x + 0.3 * c) * np.cos(0.07 * y) + 0.05 * z - 0.03 * x * (c == 1) + 0.02 * rng.standard_normal((d, h, w)))
        comps.append(a.astype(np.float32))
    comps[1][rng.random((d, h, w)) < 0.03] = np.nan
    z0, y0, x0 = (int(rng.integers(0, n)) for n in (d, h, w))
    comps[2][z0:z0 + max(1, d // 4), y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 4)] = np.nan
    axis = int(np.argmax((d, h, w)))
    if (d, h, w)[axis] > r + 2:
        slab = [slice(None)] * 3
        slab[axis] = slice(1, 1 + r)
        comps[0][tuple(slab)] = np.nan
    return comps


def check_stats(got, want):
    for k in ("defined", "folded", "lost", "thin"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("vol_min", "vol_max", "eq_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])
    assert abs(got["vol_sum"] - want["vol_sum"]) <= 1e-9 * max(1.0, want["vol_abs_sum"]), (got["vol_sum"], want["vol_sum"])


def in_a_larger_container(f3d, comps, r, min_count, mask=ALL, stats=True, null_unselected=True):
    """f3d_window_strain on a box in the corner of NaN-poisoned containers three columns, two rows and a plane larger: the whole
    output containers (sentinel-filled before the call) and the statistics"""
    d, h, w = comps[0].shape
    cdims = (w + 3, h + 2, d + 1)
    fn = f3d._window_strain_entry()
    box = f3d.Containers(*cdims)
    try:
        ins = [box.new(a) for a in comps]
        outs = [box.alloc(fill=SENTINEL) for _ in NAMES]
        box.set_current()
        arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, GROUP_OF)]
        st = f3d.WindowStrainStats() if stats else None
        f3d.check(fn(*ins, (f3d._dp * len(arr))(*arr), mask, r, min_count, w, h, d, st), "f3d_window_strain")
        f3d.sync()
        full = [box.download(p, cdims) for p in outs]
    finally:
        box.free()
    return full, (st.as_dict() if stats else None)


def check_box(full, want, dims, what):
    """the box equals `want` bit for bit (None: it still holds the sentinel) and nothing was written outside it"""
    w, h, d = dims
    inside = np.zeros(full.shape, bool)
    inside[:d, :h, :w] = True
    assert (full[~inside].view(np.uint32) == 0x7F7F7F7F).all(), f"{what}: written outside the box"
    got = full[:d, :h, :w]
    if want is None:
        assert (got.view(np.uint32) == 0x7F7F7F7F).all(), f"{what}: written although not selected"
    else:
        differ = int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want)))))
        assert same_bits(got, want), f"{what}: {differ} of {want.size} differ"


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_strain_equals_the_restatement_bit_for_bit(f3d, dims, r):
    w, h, d = dims
    d = {"run-r": 32 - r, "run+r": 32 + r}.get(d, d)
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    comps = displacement(rng, w, h, d, r)
    min_count = 4                      # the least a plane needs, so that the determinant decides which windows are thin
    want, want_stats = window_strain_ref(*comps, r, min_count)
    full, st = in_a_larger_container(f3d, comps, r, min_count)
    for name, got in zip(NAMES, full):
        check_box(got, want[name], (w, h, d), f"{dims} r={r} {name}")
    check_stats(st, want_stats)
    total = w * h * d
    assert st["defined"] + st["lost"] + st["thin"] == total
    if total > 5000:
        assert st["defined"] > total // 2 and st["lost"] > 0 and st["thin"] > 0


def test_statistics_of_volumes_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, np.float32)
    got = f3d.window_strain(nan, nan, nan, radius=2)
    st = got["stats"]
    assert st["defined"] == 0 and st["lost"] == 60 and st["thin"] == 0 and st["folded"] == 0 and st["vol_sum"] == 0
    assert np.isnan(st["vol_min"]) and np.isnan(st["vol_max"]) and np.isnan(st["eq_max"])
    assert set(got) == set(NAMES[:8]) | {"stats"} and all(np.isnan(got[n]).all() for n in NAMES[:8])
    one = np.zeros((1, 1, 1), np.float32)           # one point: present, and no plane through it
    st = f3d.window_strain(one, one, one, radius=1, min_count=1, fields="grad")["stats"]
    assert st["defined"] == 1 and st["lost"] == 0 and st["thin"] == 0 and st["vol_min"] == 0.0


@pytest.mark.parametrize("r", (1, 3))
def test_every_group_writes_exactly_its_outputs(f3d, r):
    w, h, d = 70, 19, 6
    comps = displacement(np.random.default_rng(11), w, h, d, r)
    min_count = default_min_count(r)
    want, want_stats = window_strain_ref(*comps, r, min_count)
    for mask in (1, 2, 4, 8, ALL):
        for stats, null_unselected in ((False, False), (True, True)) if mask != ALL else ((True, True),):
            full, st = in_a_larger_container(f3d, comps, r, min_count, mask, stats, null_unselected)
            for name, group, got in zip(NAMES, GROUP_OF, full):
                check_box(got, want[name] if mask & group else None, (w, h, d), f"mask {mask} stats {stats} {name}")
            if stats:
                check_stats(st, want_stats)          # vol and eq feed the statistics whether or not they are stored


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._window_strain_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w = (box.new(np.zeros((8, 8, 8), np.float32)) for _ in range(3))
        outs = [box.alloc(fill=SENTINEL) for _ in NAMES]
        box.set_current()

        def call(ins, o, mask, r=2, k=4, dims=(8, 8, 8)):
            return fn(*ins, (f3d._dp * 17)(*o) if o is not None else None, mask, r, k, *dims, None)

        def swapped(i, p):
            o = list(outs)
            o[i] = p
            return o

        bad = [
            (((0, v, w), outs, ALL), {}),                         # null inputs
            (((u, 0, w), outs, ALL), {}),
            (((u, v, 0), outs, ALL), {}),
            (((u, v, w), None, ALL), {}),                         # no output array
            (((u, v, w), swapped(0, 0), 1), {}),                  # null selected outputs
            (((u, v, w), swapped(16, 0), 8), {}),
            (((u, v, w), outs, 0), {}),                           # nothing selected
            (((u, v, w), outs, 16), {}),                          # unknown bit
            (((u, v, w), outs, ALL), {"r": 0}),                   # radius outside 1 .. 3
            (((u, v, w), outs, ALL), {"r": 4}),
            (((u, v, w), outs, ALL), {"k": 0}),                   # min_count outside 1 .. (2r+1)^3
            (((u, v, w), outs, ALL), {"r": 1, "k": 28}),
            (((u, v, w), outs, ALL), {"k": 126}),
            (((u, v, w), swapped(3, v), 2), {}),                  # a selected output that is an input
            (((u, v, w), swapped(9, u), 8), {}),
            (((u, v, w), swapped(8, outs[0]), ALL), {}),          # two equal selected outputs
            (((u, v, w), outs, ALL), {"dims": (0, 8, 8)}),        # empty, and larger than the container
            (((u, v, w), outs, ALL), {"dims": (8, 8, 9)}),
        ]
        for args, kw in bad:
            assert call(*args, **kw) == 1, (args[-1], kw)
            assert b"f3d_window_strain" in hip.f3d_last_error()
        f3d.sync()
        for p in outs:                                            # a refused call writes nothing
            assert (box.download(p, (8, 8, 8)).view(np.uint32) == 0x7F7F7F7F).all()
        # an input or a shared container as an UNSELECTED output is fine, and so are the ends of the ranges
        assert call((u, v, w), swapped(8, u), 7) == 0
        assert call((u, v, w), swapped(0, outs[8]), 8) == 0
        assert call((u, v, w), outs, ALL, r=3, k=343) == 0
        assert call((u, v, w), outs, ALL, r=1, k=27) == 0
        f3d.sync()
    finally:
        box.free()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def solved(f3d):
    """the flow of the synthetic 48 x 40 x 24 pair, and OpticalFlow.window_strain of it at radius 2 with every group"""
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        uvw = flow.download()
        got = flow.window_strain(radius=2, fields=("vol", "eq", "grad"))
        default = flow.window_strain()
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), uvw))
        flow.window_strain_end()
    finally:
        flow.destroy()
    return (w, h, d), (f0, f1), uvw, got, default


def test_window_strain_of_a_solved_flow(f3d, solved):
    dims, _, uvw, got, default = solved
    hand = f3d.window_strain(*uvw, radius=2, fields=("vol", "eq", "grad"))
    assert set(got) == set(hand) == {"vol", "eq", "stats"} | set(NAMES[8:])
    for n in hand:
        if n != "stats":
            assert same_bits(got[n], hand[n]), n
    assert got["stats"] == hand["stats"]
    want, want_stats = window_strain_ref(*uvw, 2)                      # and both equal the restatement
    for n in hand:
        if n != "stats":
            assert same_bits(got[n], want[n]), n
    check_stats(got["stats"], want_stats)
    assert got["stats"]["defined"] > 0.9 * dims[0] * dims[1] * dims[2]
    hand = f3d.window_strain(*uvw)                                     # radius 2, vol + e + eq
    assert set(default) == set(NAMES[:8]) | {"stats"} and default["stats"] == hand["stats"]
    assert all(same_bits(default[n], hand[n]) for n in NAMES[:8])


# ---- bin/flow3d --window-strain ------------------------------------------------------------------------------------------------------------------

LINE = re.compile(r"window strain \(r=(\d+)\) frame (\d+) -> frame (\d+): vol min/mean/max (\S+)/(\S+)/(\S+), eq max (\S+), (\d+) folded, "
                  r"(\d+) thin, (\d+) lost of (\d+) voxels")


def test_cli_window_strain_equals_the_binding(solved, tmp_path):
    (w, h, d), frames, _, got, _ = solved
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(np.float32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent",
            "--frames", *paths, "--out", str(tmp_path / "ws"), "--window-strain", "vol,eq,grad", "--window-radius", "2"]
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    suffix = f"-{w}-{h}-{d}.raw"
    for n in ("vol", "eq") + NAMES[8:]:
        assert same_bits(np.fromfile(str(tmp_path / f"ws_wstrain-{n}{suffix}"), np.float32).reshape(d, h, w), got[n]), n
    assert not os.path.exists(tmp_path / f"ws_wstrain-exx{suffix}")
    lines = LINE.findall(run.stdout)
    assert len(lines) == 1
    m, st = lines[0], got["stats"]
    assert (int(m[0]), int(m[1]), int(m[2])) == (2, 0, 1) and int(m[10]) == w * h * d
    assert (int(m[7]), int(m[8]), int(m[9])) == (st["folded"], st["thin"], st["lost"])
    for txt, val in ((m[3], st["vol_min"]), (m[4], st["vol_sum"] / st["defined"]), (m[5], st["vol_max"]), (m[6], st["eq_max"])):
        assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


@pytest.mark.parametrize("extra", [["--window-strain", "vol,g"], ["--window-radius", "2"], ["--window-strain", "vol", "--window-radius", "4"],
                                   ["--window-strain", "vol", "--window-radius", "1", "--window-min-count", "28"],
                                   ["--window-strain", "vol", "--partial"], ["--window-strain", "vol", "--concurrent", "2"]])
def test_cli_bad_options_exit_with_64(tmp_path, extra):
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64 and "usage" in run.stdout
    assert not any("wstrain" in n or "flow-" in n for n in os.listdir(tmp_path))
