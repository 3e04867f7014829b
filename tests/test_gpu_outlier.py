"""f3d_validate_displacement on the GPU against its numpy restatement (tests/outlier_ref.py), never against itself: the stored r and
the validated displacement bit for bit (NaN where NaN, the sign of zero included), the counts exactly, in containers three columns,
two rows and a plane larger than the box.  The margin of the INPUTS holds a finite sentinel (byte 0x7F, 3.39e38), not NaN: a NaN margin
that was wrongly read would pass for an absent neighbour and hide the bug.  The outputs are sentinel-filled too, and the margin and
the unselected outputs must still hold the sentinel afterwards.  Then the refusals, the fill passes, OpticalFlow.validate of a solved
flow, and bin/flow3d --validate --use-validated in a pipelined sequence.

Shapes: a wave covers 64 x, a workgroup 4 rows, a run 32 planes; the list has sizes of one, below, at and one above those, and
330 x 48 x 100, whose 6 * 12 * 4 = 288 workgroup partials make every thread of the fold merge at least one.  Step 16 exceeds some axes
of every shape but the last: all neighbours along those axes are outside."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import outlier_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
F32 = np.float32
SENTINEL = 0x7F      # byte fill: 0x7F7F7F7F = 3.39e38, finite
SENTINEL_BITS = 0x7F7F7F7F
WEIGHT_MIN = 0.75
EPS = 0.1
BIG = (330, 48, 100)
SHAPES = [(1, 1, 1), (2, 1, 1), (3, 3, 3), (64, 1, 1), (65, 5, 4), (7, 6, 5), (70, 24, 20), (130, 9, 33), BIG]
STEPS = (1, 2, 4, 16)
KINDS = ("noise", "holes", "ties", "weight", "absent")
R, D = 1, 2
# every mode, min_neighbours and threshold with each other; the selection and the statistics rotate beneath them so that every
# (fields, stats) pair meets every mode
COMBOS = [(mode, k, thr, (R | D, R, D)[i % 3], (i // 3) % 2 == 0)
          for i, (mode, k, thr) in enumerate(itertools.product((ref.MARK, ref.REPLACE), (1, 9, 26), (0.0, 2.0, np.inf)))]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    """equal as numbers, NaN where NaN, and the same sign everywhere else (zeros included)"""
    nan = np.isnan(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a)[~nan], np.signbit(b)[~nan])


def case_inputs(dims, kind):
    """u, v, w (and a weight) of shape [d, h, w] for one of the input kinds"""
    w, h, d = dims
    rng = np.random.default_rng(w * 7919 + h * 31 + d)
    u, v, ww = (rng.normal(m, 1.5, (d, h, w)).astype(F32) for m in (2.0, -1.0, 0.5))
    weight = None
    if kind == "holes":
        pick = rng.random((d, h, w))
        u[pick < 0.04] = np.nan
        v[(pick >= 0.04) & (pick < 0.07)] = np.nan
        ww[(pick >= 0.07) & (pick < 0.10)] = np.nan
        for a in (u, v, ww):
            a[: max(1, d // 3), : max(1, h // 2), w - max(1, w // 4):] = np.nan          # a NaN block touching three faces
    elif kind == "ties":
        u, v, ww = (rng.choice(np.array([-0.0, 0.0, 0.25, -0.25, 1.0], F32), size=(d, h, w)) for _ in range(3))
    elif kind == "weight":
        weight = rng.choice(np.array([0.0, 0.5, WEIGHT_MIN, np.nextafter(F32(WEIGHT_MIN), F32(0)), 0.9, 1.0, np.nan, -np.inf, np.inf], F32),
                            size=(d, h, w))
        u[rng.random((d, h, w)) < 0.05] = np.nan
    elif kind == "absent":
        weight = np.full((d, h, w), np.nan, F32)
    return u, v, ww, weight


class Device:
    """the inputs of one case in sentinel-margined containers, and four output containers"""

    def __init__(self, f3d, u, v, w, weight):
        self.f3d, (self.d, self.h, self.w) = f3d, u.shape
        self.cdims = (self.w + 3, self.h + 2, self.d + 1)
        self.fn = f3d._validate_entry()
        self.box = f3d.Containers(*self.cdims)
        self.p = [self.box.new(a, fill=SENTINEL) for a in (u, v, w)]
        self.pw = self.box.new(weight, fill=SENTINEL) if weight is not None else 0
        self.outs = [self.box.alloc() for _ in range(4)]
        self.box.set_current()

    def call(self, step, threshold, min_neighbours, mode, fields, stats=True, weight_min=WEIGHT_MIN):
        """the four whole output containers (sentinel-filled before the call) and the statistics or None"""
        hip = self.f3d.hip()
        for o in self.outs:
            self.f3d.check(hip.f3d_memset2d(o, self.box.pitch, SENTINEL, self.box.pitch, self.cdims[1] * self.cdims[2]), "f3d_memset2d")
        st = self.f3d.ValidateStats() if stats else None
        self.f3d.check(self.fn(*self.p, self.pw, weight_min, step, EPS, threshold, min_neighbours, mode, (C.c_uint64 * 4)(*self.outs),
                               fields, self.w, self.h, self.d, st), "f3d_validate_displacement")
        self.f3d.sync()
        return [self.box.download(o, self.cdims) for o in self.outs], st

    def free(self):
        self.box.free()


def check_call(dev, got, st, want, fields, label):
    d, h, w = dev.d, dev.h, dev.w
    inside = np.zeros((d + 1, h + 2, w + 3), bool)
    inside[:d, :h, :w] = True
    selected = [bool(fields & R)] + [bool(fields & D)] * 3
    for full, exp, sel, name in zip(got, want[:4], selected, "ruvw"):
        assert (bits(full)[~inside] == SENTINEL_BITS).all(), f"{label}: {name} written outside the box"
        if sel:
            assert same(full[:d, :h, :w], exp), f"{label}: {name} differs at {int((~np.isclose(full[:d, :h, :w], exp, 0, 0, True)).sum())} voxels"
        else:
            assert (bits(full) == SENTINEL_BITS).all(), f"{label}: the unselected {name} was written"
    if st is not None:
        ws = want[4]
        got_counts = {k: getattr(st, k) for k in ("present", "tested", "outliers", "replaced", "undefined")}
        assert got_counts == {k: ws[k] for k in got_counts}, label
        assert same(np.array([st.r_max], F32), np.array([ws["r_max"]], F32)), (label, st.r_max, ws["r_max"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_against_the_restatement(f3d, dims, kind):
    w, h, d = dims
    u, v, ww, weight = case_inputs(dims, kind)
    # the large shape is there for the fold of the partials: one step per kind keeps its restatement within seconds
    steps = (STEPS[KINDS.index(kind) % 4],) if dims == BIG else STEPS
    dev = Device(f3d, u, v, ww, weight)
    try:
        for step in steps:
            prepared = ref.prepare(u, v, ww, weight, WEIGHT_MIN, step, EPS)
            present, k = prepared[1], prepared[2]
            if kind == "holes" and w * h * d >= 200 and step == 1:                  # both parities of k among the tested voxels
                assert {x % 2 for x in k[present & (k >= 1)].tolist()} == {0, 1}
                if w * h * d > 30000:                                                # and k from 0 (inside the block) to 26
                    assert set(k.ravel().tolist()) >= {0} | set(range(4, 27))
            if step == 16 and min(dims) <= 16:                                       # an axis without any neighbour: 8 are left at most
                assert k.max() <= 8
            for n, (mode, min_neighbours, threshold, fields, stats) in enumerate(COMBOS):
                want = ref.classify(prepared, threshold, min_neighbours, mode)
                label = f"{dims} {kind} step {step} mode {mode} k>={min_neighbours} thr {threshold} fields {fields} stats {stats}"
                got, st = dev.call(step, threshold, min_neighbours, mode, fields, stats)
                check_call(dev, got, st, want, fields, label)
                if n == 0:                                                           # two calls, identical bytes and statistics
                    again, st2 = dev.call(step, threshold, min_neighbours, mode, fields, stats)
                    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again)) and bytes(st) == bytes(st2), label
                if kind == "absent":
                    assert want[4]["present"] == 0 and np.isnan(want[4]["r_max"])
                    assert all(np.isnan(g[:d, :h, :w]).all() for g, sel in zip(got, [fields & R] + [fields & D] * 3) if sel)
                if threshold == np.inf:
                    assert want[4]["outliers"] == 0
                if mode == ref.MARK:
                    assert want[4]["replaced"] == 0
        for a, p in zip((u, v, ww), dev.p):                                          # the inputs are not touched
            assert np.array_equal(bits(dev.box.download(p, dims)), bits(a))
    finally:
        dev.free()


def test_the_weight_at_the_minimum_is_present_and_one_ulp_below_is_not(f3d):
    dims = (70, 24, 20)
    u, v, ww, weight = case_inputs(dims, "weight")
    res = f3d.validate_displacement(u, v, ww, weight=weight, weight_min=WEIGHT_MIN, threshold=np.inf, min_neighbours=26, mode="mark")
    at, below = weight == F32(WEIGHT_MIN), weight == np.nextafter(F32(WEIGHT_MIN), F32(0))
    ok = ~np.isnan(u)
    assert at.any() and below.any()
    assert not np.isnan(res["u"][at & ok]).any() and np.isnan(res["u"][below]).all()
    assert np.isnan(res["u"][np.isnan(weight) | (weight == -np.inf)]).all() and not np.isnan(res["u"][(weight == np.inf) & ok]).any()
    # without a weight a NaN weight_min is fine
    plain = f3d.validate_displacement(u, v, ww, weight_min=float("nan"))
    want = ref.validate(u, v, ww)
    assert all(same(plain[n], e) for n, e in zip("ruvw", want[:4]))


def test_refusals(f3d):
    hip = f3d.hip()
    fn = f3d._validate_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        u, v, w, m = (box.new(np.ones((8, 8, 8), F32)) for _ in range(4))
        o = [box.alloc(fill=SENTINEL) for _ in range(4)]
        box.set_current()
        st = f3d.ValidateStats()
        st.present = 77
        nan, inf = float("nan"), float("inf")
        arr = lambda *p: (C.c_uint64 * 4)(*p)

        def args(**kw):
            a = dict(u=u, v=v, w=w, weight=0, weight_min=0.5, step=1, eps=0.1, threshold=2.0, k=9, mode=2, out=arr(*o), fields=3,
                     dims=(8, 8, 8))
            a.update(kw)
            return (a["u"], a["v"], a["w"], a["weight"], a["weight_min"], a["step"], a["eps"], a["threshold"], a["k"], a["mode"], a["out"],
                    a["fields"], *a["dims"], C.byref(st))

        bad = [args(u=0), args(v=0), args(w=0),                                                     # a null input
               args(out=arr(0, o[1], o[2], o[3])), args(out=arr(o[0], o[1], 0, o[3])), args(out=None),   # a null selected output
               args(fields=0), args(fields=4), args(fields=7),
               args(mode=0), args(mode=3),
               args(step=0), args(step=17),
               args(k=0), args(k=27),
               args(eps=nan), args(eps=inf), args(eps=0.0), args(eps=-0.1),
               args(threshold=nan), args(threshold=-1.0),
               args(weight=m, weight_min=nan),
               args(out=arr(u, o[1], o[2], o[3])), args(out=arr(o[0], o[1], w, o[3])),                  # an output that is an input
               args(weight=m, out=arr(m, o[1], o[2], o[3])), args(weight=m, out=arr(o[0], o[1], o[2], m)),   # the weight included
               args(out=arr(o[0], o[0], o[2], o[3])), args(out=arr(o[0], o[1], o[2], o[1])),            # two outputs alike
               args(dims=(0, 8, 8)), args(dims=(8, 0, 8)), args(dims=(8, 8, 0)),
               args(dims=(9, 8, 8))]                                                                  # larger than the container
        for a in bad:
            assert fn(*a) == 1, a
            assert b"f3d_validate_displacement" in hip.f3d_last_error(), hip.f3d_last_error()
        f3d.sync()
        assert st.present == 77                                                                       # a refused call writes nothing
        for p in o:
            assert (bits(box.download(p, (8, 8, 8))) == SENTINEL_BITS).all()
        # accepted: threshold +inf; an unselected output may be null or anything; a NaN weight_min without a weight
        assert fn(*args(threshold=inf)) == 0 and st.outliers == 0 and st.present == 512
        assert fn(*args(fields=1, out=arr(o[0], 0, 0, 0))) == 0 and fn(*args(fields=2, out=arr(u, o[1], o[2], o[3]))) == 0
        assert fn(*args(weight_min=nan)) == 0 and fn(*args(weight=m, weight_min=-inf)) == 0 and st.present == 512
        f3d.sync()
    finally:
        box.free()


def test_fill_passes_close_a_block(f3d):
    w, h, d = 70, 24, 20
    u, v, ww, _ = case_inputs((w, h, d), "noise")
    for a in (u, v, ww):
        a[8:13, 10:15, 30:35] = np.nan                                               # 5 x 5 x 5 in the interior
    first = ref.validate(u, v, ww, threshold=3.0, min_neighbours=9, mode=ref.REPLACE)
    fu, fv, fw, replaced, undefined, history = ref.fill(*first[1:4], 3)
    counts = [first[4]["undefined"]] + history
    print("undefined after each pass:", counts)
    assert all(b < a for a, b in zip(counts, counts[1:])) and counts[-1] == 0 and 0 < counts[0] < 125
    got = f3d.validate_displacement(u, v, ww, threshold=3.0, min_neighbours=9, mode="replace", fill_passes=3)
    assert same(got["r"], first[0]) and all(same(got[n], e) for n, e in zip("uvw", (fu, fv, fw)))
    exp = dict(first[4], replaced=first[4]["replaced"] + replaced, undefined=0)
    assert {k: got["stats"][k] for k in exp if k != "r_max"} == {k: exp[k] for k in exp if k != "r_max"}
    assert F32(got["stats"]["r_max"]) == exp["r_max"]
    # by hand, one call after the other: the restatement applied four times
    hand = first
    for _ in range(3):
        hand = ref.validate(*hand[1:4], threshold=np.inf, min_neighbours=9, mode=ref.REPLACE)
    assert all(same(got[n], e) for n, e in zip("uvw", hand[1:4]))
    # fewer passes than it takes, and none
    one = f3d.validate_displacement(u, v, ww, threshold=3.0, mode="replace", fill_passes=1)
    assert one["stats"]["undefined"] == counts[1] and int(np.isnan(one["u"]).sum()) == counts[1]
    none = f3d.validate_displacement(u, v, ww, threshold=3.0, mode="replace")
    assert none["stats"]["undefined"] == counts[0] and all(same(none[n], e) for n, e in zip("ruvw", first[:4]))
    # under "mark" the fill is what repairs: the outliers no longer vote
    marked = f3d.validate_displacement(u, v, ww, threshold=3.0, mode="mark", fill_passes=8)
    m = ref.validate(u, v, ww, threshold=3.0, mode=ref.MARK)
    mu, mv, mw, mrep, mund, _ = ref.fill(*m[1:4], 8)
    assert all(same(marked[n], e) for n, e in zip("uvw", (mu, mv, mw)))
    assert marked["stats"]["replaced"] == mrep and marked["stats"]["undefined"] == mund == 0


def test_validate_of_a_solved_flow(f3d):
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        u, v, ww = flow.download()
        with pytest.raises(f3d.F3dError, match="match"):                        # a mask needs the zncc of a match of this pair
            flow.validate(min_zncc=0.5)
        for kw in (dict(), dict(step=4, mode="mark", threshold=1.0), dict(step=2, min_neighbours=20, eps=0.01, fill_passes=2)):
            got = flow.validate(**kw)
            hand = f3d.validate_displacement(u, v, ww, **kw)
            assert all(np.array_equal(bits(got[n]), bits(hand[n])) for n in "ruvw"), kw
            assert got["stats"] == hand["stats"] and got["stats"]["present"] == w * h * d
            want = ref.validate(u, v, ww, None, 0.8, kw.get("step", 1), kw.get("eps", 0.1), kw.get("threshold", 2.0),
                                kw.get("min_neighbours", 9), ref.MODES[kw.get("mode", "replace")])
            if not kw.get("fill_passes"):
                assert all(same(got[n], e) for n, e in zip("ruvw", want[:4]))
        only_r = flow.validate(fields="r")
        assert set(only_r) == {"r", "stats"} and np.array_equal(bits(only_r["r"]), bits(f3d.validate_displacement(u, v, ww)["r"]))
        zncc = flow.match(fields="zncc")["zncc"]
        level = float(np.nanpercentile(zncc, 30))
        for fill_passes in (0, 3):
            masked = flow.validate(min_zncc=level, fill_passes=fill_passes)
            hand = f3d.validate_displacement(u, v, ww, weight=zncc, weight_min=level, fill_passes=fill_passes)
            assert all(np.array_equal(bits(masked[n]), bits(hand[n])) for n in "ruvw") and masked["stats"] == hand["stats"]
            with np.errstate(invalid="ignore"):
                assert masked["stats"]["present"] == int((zncc >= F32(level)).sum()) < w * h * d
        assert masked["stats"]["undefined"] < flow.validate(min_zncc=level)["stats"]["undefined"]
        # a new solve makes the old zncc stale; the trajectory is a source too, but has no mask
        flow.compute_resident(silent=True, **KW)
        with pytest.raises(f3d.F3dError, match="match"):
            flow.validate(min_zncc=0.5)
        flow.trajectory_begin()
        flow.trajectory_append()
        traj = flow.validate(source="trajectory", step=2)
        assert all(np.array_equal(bits(traj[n]), bits(e)) for n, e in zip("ruvw", ref.validate(u, v, ww, step=2)[:4]))
        flow.match(fields="zncc")
        with pytest.raises(f3d.F3dError, match="trajectory"):
            flow.validate(source="trajectory", min_zncc=0.5)
        flow.validate_end()
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), (u, v, ww)))
    finally:
        flow.destroy()


# ---- bin/flow3d --validate --use-validated in a pipelined sequence --------------------------------------------------------------------------

LINE = re.compile(r"validate frame (\d+) -> frame (\d+) \(replace, step 1\): (\d+) tested, (\d+) outliers, (\d+) replaced, (\d+) undefined, "
                  r"r max (\S+) of (\d+) voxels")


def test_cli_validate_in_a_sequence(f3d, tmp_path):
    w, h, d = 48, 40, 24
    s0, s1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate([s0, s1, s0]):
        p = str(tmp_path / f"f{i}.raw")
        f.astype(F32).tofile(p)
        paths.append(p)
    args = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    read = lambda name: np.fromfile(str(tmp_path / name), F32).reshape(d, h, w)
    raw = lambda name: open(tmp_path / name, "rb").read()

    def run(tag, extra):
        r = subprocess.run(args + ["--out", str(tmp_path / tag)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    so = run("v", ["--match", "zncc", "--validate", "replace", "--validate-min-zncc", "0.5", "--validate-fill", "2", "--use-validated",
                   "--strain", "vol"])
    plain = run("p", ["--match", "zncc", "--strain", "vol"])
    lines = LINE.findall(so)
    assert len(lines) == 2
    differs = 0
    for k in range(2):
        for name in [f"flow-{c}" for c in "uvw"] + ["match-zncc"]:
            assert raw(f"v_{k}_{name}{suffix}") == raw(f"p_{k}_{name}{suffix}"), f"{name} of pair {k}"
        flow_k = [read(f"v_{k}_flow-{c}{suffix}") for c in "uvw"]
        zncc = read(f"v_{k}_match-zncc{suffix}")
        want = f3d.validate_displacement(*flow_k, weight=zncc, weight_min=0.5, fill_passes=2)
        for n in "ruvw":
            assert np.array_equal(bits(read(f"v_{k}_validated-{n}{suffix}")), bits(want[n])), f"validated-{n} of pair {k}"
        strain = f3d.flow_strain(want["u"], want["v"], want["w"], fields="vol")
        assert np.array_equal(bits(read(f"v_{k}_strain-vol{suffix}")), bits(strain["vol"])), f"strain of pair {k}"
        differs += raw(f"v_{k}_strain-vol{suffix}") != raw(f"p_{k}_strain-vol{suffix}")
        m, st = lines[k], want["stats"]
        assert (int(m[0]), int(m[1])) == (k, k + 1) and int(m[7]) == w * h * d
        assert [int(x) for x in m[2:6]] == [st["tested"], st["outliers"], st["replaced"], st["undefined"]]
        assert float(m[6]) == pytest.approx(st["r_max"], rel=1e-5)
        assert st["present"] < w * h * d                                          # the mask took something out
    assert differs                                                              # the strain is of the validated field, not of the raw one
    # without --use-validated the strain is the raw one, and the lines of the other features stand as they were
    so = run("n", ["--match", "zncc", "--validate", "mark", "--validate-step", "2", "--strain", "vol"])
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("strain frame", "match frame"))]
    assert keep(so) == keep(plain) and len(keep(so)) == 4
    for k in range(2):
        assert raw(f"n_{k}_strain-vol{suffix}") == raw(f"p_{k}_strain-vol{suffix}")
        flow_k = [read(f"n_{k}_flow-{c}{suffix}") for c in "uvw"]
        want = f3d.validate_displacement(*flow_k, step=2, mode="mark")
        assert all(np.array_equal(bits(read(f"n_{k}_validated-{n}{suffix}")), bits(want[n])) for n in "ruvw")
    assert not any(n.startswith("p_") and "validated" in n for n in os.listdir(tmp_path))
