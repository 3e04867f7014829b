"""Local correlation on the GPU: f3d_local_correlation against its numpy restatement (tests/correlation_ref.py) bit for bit with its
statistics, in NaN-poisoned containers larger than the box; the field selection and the refusals of the entry; the driver's match
quality of a solved flow (OpticalFlow.match) against carry_field + local_correlation by hand; and bin/flow3d --match against the
binding.

Shapes: the kernel's tile is 32 x 8 voxels of a plane and a run is 32 planes, so the list holds widths and heights at the tile edges
and one off, depths of a run -r and +r planes and of three runs and a remainder, next to the shapes every derived field is tried on."""
import os
import re
import subprocess

import numpy as np
import pytest

from correlation_ref import local_correlation, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
SENTINEL = 0x7F      # byte fill of the outputs: 0x7F7F7F7F = 3.39e38
THRESHOLD = 0.85    # the volumes of pair_of_volumes correlate at 0.84: about half of the defined voxels are below
RADII = (1, 2, 3, 4)
SHAPES = [(1, 1, 1), (2, 2, 2), (31, 5, 3), (32, 5, 3), (33, 5, 3), (63, 5, 3), (64, 5, 3), (65, 5, 3), (9, 7, 3), (9, 8, 3),
          (9, 9, 3), (9, 15, 3), (9, 16, 3), (9, 17, 3), (64, 64, 1), (37, 23, 11), (584, 388, 5), (5, 4, 101), (7, 5, "run-r"),
          (7, 5, "run+r"), (257, 65, 33)]


def pair_of_volumes(rng, w, h, d):
    """correlated noise with scattered NaNs in either volume, a NaN block, and two blocks of flat windows: both volumes constant in
    the corner at the origin, a alone constant somewhere"""
    shape = (d, h, w)
    a = rng.uniform(0, 255, shape).astype(np.float32)
    b = (np.float32(0.6) * a + rng.uniform(0, 100, shape).astype(np.float32)).astype(np.float32)
    a[:12, :12, :12] = np.float32(17.25)
    b[:12, :12, :12] = np.float32(-3.5)
    z0, y0, x0 = (int(rng.integers(0, n)) for n in shape)
    a[z0:z0 + 12, y0:y0 + 12, x0:x0 + 12] = np.float32(255.3)
    pick = rng.random(shape)
    a[pick < 0.03] = np.nan
    b[pick > 0.97] = np.nan
    z0, y0, x0 = (int(rng.integers(0, n)) for n in shape)
    b[z0:z0 + max(1, d // 4), y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 4)] = np.nan
    return a, b


def check_stats(got, want):
    for k in ("defined", "lost", "below"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("zncc_min", "rmsd_max"):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or np.float32(got[k]) == np.float32(want[k]), (k, got[k], want[k])
    assert abs(got["zncc_sum"] - want["zncc_sum"]) <= 1e-9 * max(1.0, want["zncc_abs_sum"]), (got["zncc_sum"], want["zncc_sum"])


def in_a_larger_container(f3d, a, b, r, mask=3, stats=True, null_unselected=True):
    """f3d_local_correlation on a box in the corner of NaN-poisoned containers three columns, two rows and a plane larger: the whole
    output containers (sentinel-filled before the call) and the statistics"""
    d, h, w = a.shape
    cdims = (w + 3, h + 2, d + 1)
    fn = f3d._correlation_entry()
    box = f3d.Containers(*cdims)
    try:
        pa, pb = box.new(a), box.new(b)
        outs = [box.alloc(fill=SENTINEL) for _ in range(2)]
        box.set_current()
        arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, (1, 2))]
        st = f3d.CorrelationStats() if stats else None
        f3d.check(fn(pa, pb, (f3d._dp * 2)(*arr), mask, r, THRESHOLD, w, h, d, st), "f3d_local_correlation")
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
def test_local_correlation_equals_the_restatement_bit_for_bit(f3d, dims, r):
    w, h, d = dims
    d = {"run-r": 32 - r, "run+r": 32 + r}.get(d, d)
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    a, b = pair_of_volumes(rng, w, h, d)
    zncc, rmsd, want = local_correlation(a, b, r, THRESHOLD)
    (got_zncc, got_rmsd), st = in_a_larger_container(f3d, a, b, r)
    check_box(got_zncc, zncc, (w, h, d), f"{dims} r={r} zncc")
    check_box(got_rmsd, rmsd, (w, h, d), f"{dims} r={r} rmsd")
    check_stats(st, want)
    if w * h * d > 5000:
        total = w * h * d
        assert 0 < st["defined"] < total and st["lost"] > 0 and st["below"] > 0 and st["defined"] + st["lost"] < total  # some are flat


def test_statistics_of_volumes_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, np.float32)
    got = f3d.local_correlation(nan, nan, radius=2)
    st = got["stats"]
    assert st["defined"] == 0 and st["lost"] == 60 and st["below"] == 0 and st["zncc_sum"] == 0
    assert np.isnan(st["zncc_min"]) and np.isnan(st["rmsd_max"])
    assert set(got) == {"zncc", "rmsd", "stats"} and np.isnan(got["zncc"]).all() and np.isnan(got["rmsd"]).all()
    const = np.full((3, 4, 5), 2.5, np.float32)                 # present everywhere, flat everywhere
    st = f3d.local_correlation(const, const, radius=1, fields="zncc")["stats"]
    assert st["defined"] == 0 and st["lost"] == 0 and np.isnan(st["zncc_min"]) and st["rmsd_max"] == 0.0


@pytest.mark.parametrize("r", (1, 4))
def test_every_subset_writes_exactly_its_outputs(f3d, r):
    w, h, d = 70, 19, 6
    a, b = pair_of_volumes(np.random.default_rng(11), w, h, d)
    zncc, rmsd, want = local_correlation(a, b, r, THRESHOLD)
    for mask in (1, 2, 3):
        for stats in (False, True):
            for null_unselected in (False, True):
                full, st = in_a_larger_container(f3d, a, b, r, mask, stats, null_unselected)
                what = f"mask {mask} stats {stats} null {null_unselected}"
                check_box(full[0], zncc if mask & 1 else None, (w, h, d), what + " zncc")
                check_box(full[1], rmsd if mask & 2 else None, (w, h, d), what + " rmsd")
                if stats:
                    check_stats(st, want)          # both fields feed the statistics whether or not they are stored


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._correlation_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        a, b, o0, o1 = (box.new(np.zeros((8, 8, 8), np.float32)) for _ in range(4))
        box.set_current()

        def call(a_, b_, o, mask, r=2, threshold=0.8):
            return fn(a_, b_, (f3d._dp * 2)(*o), mask, r, threshold, 8, 8, 8, None)

        bad = [
            ((0, b, [o0, o1], 3), {}),                       # null inputs
            ((a, 0, [o0, o1], 3), {}),
            ((a, b, [0, o1], 1), {}),                        # null selected outputs
            ((a, b, [o0, 0], 3), {}),
            ((a, b, [o0, o1], 0), {}),                       # nothing selected
            ((a, b, [o0, o1], 4), {}),                       # unknown bit
            ((a, b, [o0, o1], 3), {"r": 0}),                 # radius outside 1 .. 4
            ((a, b, [o0, o1], 3), {"r": 5}),
            ((a, b, [a, o1], 1), {}),                        # a selected output that is an input
            ((a, b, [o0, b], 2), {}),
            ((a, b, [o0, o0], 3), {}),                       # two equal selected outputs
            ((a, b, [o0, o1], 3), {"threshold": float("nan")}),
        ]
        for args, kw in bad:
            assert call(*args, **kw) != 0, (args[-1], kw)
            assert b"f3d_local_correlation" in hip.f3d_last_error()
        # an input or a shared container as an UNSELECTED output is fine, and so is a against itself
        assert call(a, b, [o0, a], 1) == 0
        assert call(a, b, [o1, o1], 2) == 0
        assert call(a, a, [o0, o1], 3, r=4, threshold=float("inf")) == 0
        f3d.sync()
    finally:
        box.free()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def test_match_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        got = flow.match(fields=("warped", "zncc", "rmsd"), radius=2, threshold=0.9)
        warped, lost = f3d.carry_field(f1, u, v, ww)
        hand = f3d.local_correlation(f0, warped, radius=2, threshold=0.9)
        assert same_bits(got["warped"], warped) and same_bits(got["zncc"], hand["zncc"]) and same_bits(got["rmsd"], hand["rmsd"])
        assert got["stats"] == hand["stats"] and got["stats"]["lost"] == lost
        zncc, rmsd, want = local_correlation(f0, warped, 2, 0.9)                  # and both equal the restatement
        assert same_bits(got["zncc"], zncc) and same_bits(got["rmsd"], rmsd)
        check_stats(got["stats"], want)
        part = flow.match(fields="rmsd")                                          # radius 3, threshold 0.8
        assert set(part) == {"rmsd", "stats"}
        hand3 = f3d.local_correlation(f0, warped, fields="rmsd")
        assert same_bits(part["rmsd"], hand3["rmsd"]) and part["stats"] == hand3["stats"]
        only = flow.match(fields="warped", radius=1)
        assert set(only) == {"warped", "stats"} and same_bits(only["warped"], warped)
        # the solved flow registers the frames better than no flow at all
        unregistered = f3d.local_correlation(f0, f1, radius=2)["zncc"]
        both = ~np.isnan(got["zncc"]) & ~np.isnan(unregistered)
        solved_mean, zero_mean = float(got["zncc"][both].mean()), float(unregistered[both].mean())
        print(f"mean zncc over {int(both.sum())} voxels: {solved_mean:.4f} with the solved flow, {zero_mean:.4f} with none")
        assert both.sum() > 1000 and solved_mean > zero_mean
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), (u, v, ww)))
        # a trajectory has no match quality: frame 0 is not kept
        flow.trajectory_begin()
        ptrs = (f3d._fp * 3)(*[np.empty((d, h, w), np.float32).ctypes.data_as(f3d._fp) for _ in range(3)])
        assert f3d.host().f3d_flow_match_compute(flow._h, 1, 7, 3, 0.8, ptrs, None) != 0
        assert b"trajectory" in f3d.host().f3d_host_last_error()
        flow.match_end()
    finally:
        flow.destroy()


# ---- bin/flow3d --match ------------------------------------------------------------------------------------------------------------------------

def four_frames(f3d):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    i128 = np.load(os.path.join(ROOT, "tests", "golden", "inputs_128.npz"))
    crop = (slice(40, 40 + d), slice(40, 40 + h), slice(40, 40 + w))
    c0 = i128["frame_0"].astype(np.float32)[crop].copy()
    c1 = i128["frame_1"].astype(np.float32)[crop].copy()
    return (w, h, d), [s0, s1, c1, c0]


@pytest.fixture(scope="module")
def sequence(f3d):
    """per pair of the four frames: OpticalFlow.match at radius 2 and at the default radius between the yields of a sequence"""
    dims, frames = four_frames(f3d)
    flow = f3d.OpticalFlow()
    flow.initialize(*dims)
    out = []
    for k, fl, disp in flow.compute_sequence(frames, cumulative=True, **KW):
        out.append((flow.match(fields=("warped", "zncc", "rmsd"), radius=2), flow.match(fields=("zncc", "rmsd"))))
    flow.destroy()
    return dims, frames, out


LINE = re.compile(r"match frame (\d+) -> frame (\d+): zncc min/mean (\S+)/(\S+), (\d+) below (\S+), rmsd max (\S+), (\d+) flat, "
                  r"(\d+) lost of (\d+) voxels")


def check_line(m, stats, a, b, total):
    assert (int(m[0]), int(m[1])) == (a, b)
    assert int(m[4]) == stats["below"] and float(m[5]) == pytest.approx(0.8) and int(m[9]) == total
    assert int(m[8]) == stats["lost"] and int(m[7]) == total - stats["defined"] - stats["lost"]
    mean = stats["zncc_sum"] / stats["defined"]
    for txt, val in ((m[2], stats["zncc_min"]), (m[3], mean), (m[6], stats["rmsd_max"])):
        assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


def test_cli_match_equals_the_binding(sequence, tmp_path):
    (w, h, d), frames, out = sequence
    total = w * h * d
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(np.float32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent"]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), np.float32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, frames_, extra):
        r = subprocess.run(args + ["--frames", *frames_, "--out", str(tmp_path / tag)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    # a sequence: every pair's own flow and frames, all three fields at radius 2
    so = run("m", paths, ["--match", "warped,zncc,rmsd", "--match-radius", "2"])
    lines = LINE.findall(so)
    assert len(lines) == 3
    for k in range(3):
        for n in ("warped", "zncc", "rmsd"):
            assert same_bits(read(f"m_{k}_match-{n}{suffix}"), out[k][0][n]), f"pair {k} {n}"
        check_line(lines[k], out[k][0]["stats"], k, k + 1, total)

    # under --cumulative and beside --strain it is still the pair's match; the other options' files and lines do not change
    so = run("cm", paths, ["--cumulative", "--strain", "vol", "--match", "zncc"])
    plain = run("c", paths, ["--cumulative", "--strain", "vol"])
    lines = LINE.findall(so)
    assert len(lines) == 3
    for k in range(3):
        assert same_bits(read(f"cm_{k}_match-zncc{suffix}"), out[k][1]["zncc"]), f"cumulative pair {k}"
        assert not os.path.exists(tmp_path / f"cm_{k}_match-rmsd{suffix}") and not os.path.exists(tmp_path / f"cm_{k}_match-warped{suffix}")
        check_line(lines[k], out[k][1]["stats"], k, k + 1, total)
        for name in [f"flow-{c}" for c in "uvw"] + [f"disp-{c}" for c in "uvw"] + ["strain-vol"]:
            assert raw(f"cm_{k}_{name}{suffix}") == raw(f"c_{k}_{name}{suffix}"), f"{name} of pair {k}"
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("strain frame", "displacement frame"))]
    assert keep(so) == keep(plain) and len(keep(so)) == 6
    assert not any(n.startswith("c_") and "match" in n for n in os.listdir(tmp_path))

    # one pair, computed synchronously: tag without the pair index, the default radius
    so = run("one", paths[:2], ["--match", "rmsd,zncc"])
    lines = LINE.findall(so)
    assert len(lines) == 1
    for n in ("zncc", "rmsd"):
        assert same_bits(read(f"one_match-{n}{suffix}"), out[0][1][n]), n
    assert not os.path.exists(tmp_path / f"one_match-warped{suffix}")
    check_line(lines[0], out[0][1]["stats"], 0, 1, total)


@pytest.mark.parametrize("extra", [["--match", "zncc,ncc"], ["--match-radius", "2"], ["--match", "zncc", "--match-radius", "9"],
                                   ["--match", "zncc", "--partial"], ["--match", "zncc", "--concurrent", "2"]])
def test_cli_bad_options_exit_with_64(tmp_path, extra):
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64 and "usage" in run.stdout
    assert not any("match" in n or "flow-" in n for n in os.listdir(tmp_path))
