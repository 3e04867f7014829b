"""The normalised median test without a GPU: the vectorised numpy restatement of f3d_validate_displacement (tests/outlier_ref.py)
against a per-voxel loop that builds every neighbour list explicitly, bit for bit; what the test does on fields built of exact
(dyadic) numbers, where the bound on a repaired value follows from a median lying inside the range of its list; the generated
networks; the ABI and the binding; and the argument errors of bin/flow3d --validate."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import outlier_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    """equal as numbers, NaN where NaN, and the same sign of zero"""
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- the restatement against the loop ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [ref.MARK, ref.REPLACE], ids=["mark", "replace"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("dims", [(3, 3, 3), (7, 6, 5), (5, 1, 4)], ids=ids)
def test_the_restatement_equals_the_loop(dims, step, mode):
    w, h, d = dims
    rng = np.random.default_rng(w * 100 + h * 10 + d + step)
    u, v, ww = (rng.normal(0, 1, (d, h, w)).astype(F32) for _ in range(3))
    for a in (u, v, ww):
        a[rng.random((d, h, w)) < 0.08] = np.nan                                    # holes, one component each
    u[rng.random((d, h, w)) < 0.1] = F32(6)                                         # and some spikes
    weight = rng.choice(np.array([0.2, 0.8, 0.9, np.nan], F32), size=(d, h, w), p=[0.15, 0.3, 0.45, 0.1])
    seen = set()
    for wt in (None, weight):
        for min_neighbours in (1, 5):
            got = ref.validate(u, v, ww, wt, 0.8, step, 0.1, 1.5, min_neighbours, mode)
            want = ref.validate_loop(u, v, ww, wt, 0.8, step, 0.1, 1.5, min_neighbours, mode)
            for g, e, name in zip(got[:4], want[:4], "ruvw"):
                assert np.array_equal(bits(g), bits(e)), (name, wt is not None, min_neighbours)
            gs, es = got[4], want[4]
            assert {k: gs[k] for k in gs if k != "r_max"} == {k: es[k] for k in es if k != "r_max"}
            assert same(F32(gs["r_max"]), F32(es["r_max"]))
            seen.add((gs["outliers"] > 0, gs["replaced"] > 0))
            assert gs["undefined"] == int(np.isnan(got[1]).sum()) == int(np.isnan(got[2]).sum()) == int(np.isnan(got[3]).sum())
            assert (gs["replaced"] == 0) == (mode == ref.MARK) or w * h * d < 30
    assert w * h * d < 30 or any(o for o, _ in seen)


def test_the_median_rule_by_hand():
    # a 3 x 1 x 1 row: the middle voxel has two neighbours (even: their mean), the ends have one (odd: itself)
    u = np.array([[[1.0, 10.0, 4.0]]], F32)
    z = np.zeros_like(u)
    r, vu, vv, vw, st = ref.validate(u, z, z, step=1, eps=0.5, threshold=2.0, min_neighbours=1, mode=ref.REPLACE)
    # middle: med 2.5, residuals 1.5 1.5 -> r = 7.5 / 2 = 3.75, an outlier, replaced by 2.5; ends: med 10, rm 0, r = 9 / 0.5 and 6 / 0.5
    assert r[0, 0].tolist() == [18.0, 3.75, 12.0]
    assert vu[0, 0].tolist() == [10.0, 2.5, 10.0] and st["outliers"] == 3 and st["replaced"] == 3 and st["r_max"] == 18
    r, vu, *_ = ref.validate(u, z, z, step=1, eps=0.5, threshold=2.0, min_neighbours=2, mode=ref.MARK)
    assert np.isnan(r[0, 0, 0]) and np.isnan(r[0, 0, 2]) and r[0, 0, 1] == 3.75
    assert vu[0, 0, 0] == 1 and np.isnan(vu[0, 0, 1]) and vu[0, 0, 2] == 4          # too few neighbours: kept, untested
    # a zero median of either sign is stored as +0
    u = np.array([[[-0.0, np.nan, -0.0]]], F32)
    _, vu, *_ = ref.validate(u, z, z, min_neighbours=2, mode=ref.REPLACE)
    assert vu[0, 0, 1] == 0 and not np.signbit(vu[0, 0, 1]) and np.signbit(vu[0, 0, 0])


# ---- behaviour on exact inputs -------------------------------------------------------------------------------------------------------

G = np.array([[1, -2, 1], [-1, 1, 2], [2, 1, -1]]) / 32.0      # gradient of component c along x, y, z: dyadic, at most 1/16
BEHAVIOUR = [((70, 24, 20), 1), ((70, 24, 20), 2), ((130, 9, 33), 4)]


def exact_field(dims, seed):
    w, h, d = dims
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    f = [(G[c, 0] * x + G[c, 1] * y + G[c, 2] * z + (c - 1) * 0.5).astype(F32) for c in range(3)]
    rng = np.random.default_rng(seed)
    f[0] = f[0] + (rng.integers(0, 2, (d, h, w)) * 2 - 1).astype(F32) / F32(32)     # dyadic noise of +-1/32 in u
    return f


@pytest.mark.parametrize("dims,step", BEHAVIOUR, ids=lambda p: ids(p))
def test_clean_fields_pass_and_planted_spikes_are_found_and_repaired(dims, step):
    w, h, d = dims
    clean = exact_field(dims, w + step)
    for a in clean:                                                                  # every value is a multiple of 1/32: exact in float32
        assert np.array_equal(a * 32, np.round(a * 32)) and np.abs(a).max() < 64
    r, cu, cv, cw, st = ref.validate(*clean, step=step, eps=0.1, threshold=2.0, min_neighbours=9, mode=ref.REPLACE)
    print(f"{dims} step {step}: clean r_max {st['r_max']:.4f}, tested {st['tested']} of {w * h * d}")
    assert st["outliers"] == 0 and st["replaced"] == 0 and st["undefined"] == 0 and st["present"] == w * h * d
    assert st["r_max"] <= 2 and all(np.array_equal(bits(a), bits(b)) for a, b in zip((cu, cv, cw), clean))
    # only voxels with too few neighbours go untested: with 9 required those are the edges and corners where fewer than 9 of the 26 fit
    _, _, k = ref.neighbour_medians(clean[0], np.ones((d, h, w), bool), step)
    assert np.array_equal(np.isnan(r), k < 9) and st["tested"] == int((k >= 9).sum())

    rng = np.random.default_rng(11 * w + step)
    cand = [(z, y, x) for z in range(step, d - step) for y in range(step, h - step) for x in range(step, w - step)]
    picks = [cand[i] for i in rng.choice(len(cand), 60, replace=False)]
    field = [a.copy() for a in clean]
    planted = np.zeros((d, h, w), bool)
    for n, p in enumerate(picks):
        field[0][p] += F32(3 if n % 2 else -3)
        if n < 20:
            field[1][p] += F32(-2)
        planted[p] = True
    r, fu, fv, fw, st = ref.validate(*field, step=step, eps=0.1, threshold=2.0, min_neighbours=9, mode=ref.REPLACE)
    with np.errstate(invalid="ignore"):
        flagged = r > 2
    print(f"{dims} step {step}: {int((flagged & planted).sum())} of 60 flagged, {int((flagged & ~planted).sum())} others")
    assert np.array_equal(flagged, planted) and st["outliers"] == 60 and st["replaced"] == 60 and st["undefined"] == 0
    for c, (got, a) in enumerate(zip((fu, fv, fw), clean)):
        assert np.array_equal(bits(got[~planted]), bits(field[c][~planted]))          # everything else bit for bit
        bound = step * np.abs(G[c]).sum() + 2 / 32                                  # a median lies inside its list's range
        assert np.abs(got[planted].astype(np.float64) - a[planted]).max() <= bound, (c, bound)
    _, mu, mv, mw, sm = ref.validate(*field, step=step, eps=0.1, threshold=2.0, min_neighbours=9, mode=ref.MARK)
    assert sm["replaced"] == 0 and sm["undefined"] == 60
    assert all(np.array_equal(np.isnan(a), planted) for a in (mu, mv, mw))


def test_the_fill_closes_a_block_from_its_faces_inwards():
    f = exact_field((20, 12, 10), 3)
    for a in f:
        a[3:8, 4:9, 6:11] = np.nan
    _, u, v, w, st = ref.validate(*f, threshold=np.inf, mode=ref.REPLACE)
    assert st["outliers"] == 0 and 0 < st["undefined"] < 125 and st["replaced"] == 125 - st["undefined"]
    u, v, w, replaced, undefined, history = ref.fill(u, v, w, 5)
    assert undefined == 0 and replaced == st["undefined"] and history == sorted(history, reverse=True) and len(history) < 5
    assert not np.isnan(u).any()


# ---- generated networks, ABI, binding --------------------------------------------------------------------------------------------------

def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_validate_networks_are_current():
    """csrc/f3d_validate_nets.h is what tools/gen_median_nets.py main_validate() writes (each network checked against sorted() on inputs
    with many ties and every number of +inf pads before it is emitted)"""
    gen = load_tool("gen_median_nets")
    text, counts = gen.main_validate()
    assert counts == [292, 70]
    with open(gen.HEADER_VALIDATE) as f:
        assert f.read() == text


def test_the_kernel_is_not_built_without_nan_semantics():
    text = open(os.path.join(ROOT, "cuda-flow3d_amd", "Makefile")).read()
    lines = [l for l in text.splitlines() if "MEDIAN_FLAGS" in l and not l.lstrip().startswith("#")]
    assert lines and not any("validate" in l for l in lines)


def test_the_header_and_the_binding(f3d):
    text = open(os.path.join(ROOT, "include", "f3d.h")).read()
    for needle in ("#define F3D_VALIDATE_R 1u", "#define F3D_VALIDATE_D 2u", "#define F3D_VALIDATE_MARK 1u", "#define F3D_VALIDATE_REPLACE 2u",
                   "r_c = fabsf(d_c - med_c) / (rm_c + eps)", "0.5f * (s_{k/2-1} + s_{k/2})", "med_u + 0.f", "no mirroring"):
        assert needle in text, needle
    host = open(os.path.join(ROOT, "include", "f3d_host.h")).read()
    assert "f3d_flow_validate_compute" in host and "f3d_flow_validate_end" in host
    assert f3d.VALIDATE_MODES == {"mark": 1, "replace": 2} and f3d.VALIDATE_GROUPS == {"r": 1, "d": 2}
    assert [n for n, _ in f3d.ValidateStats._fields_] == ["present", "tested", "outliers", "replaced", "undefined", "r_max"]
    assert C.sizeof(f3d.ValidateStats) == 48
    assert callable(f3d.validate_displacement) and hasattr(f3d.OpticalFlow, "validate") and hasattr(f3d.OpticalFlow, "validate_end")
    with pytest.raises(ValueError):
        f3d._validate_mode("smooth")
    z = np.zeros((2, 2, 2), F32)
    with pytest.raises(ValueError):
        f3d.validate_displacement(z, z, z, fill_passes=1, fields=("r",))


# ---- bin/flow3d --validate: refusals that need no GPU ----------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,needle", [(["--validate-threshold", "2"], "need --validate"),
                                          (["--validate-fill", "3"], "need --validate"),
                                          (["--use-validated", "--strain", "vol"], "--use-validated needs --validate"),
                                          (["--validate", "replace", "--validate-min-zncc", "0.5"], "needs --match"),
                                          (["--validate", "replace", "--validate-min-zncc", "0.5", "--match", "rmsd"], "needs --match"),
                                          (["--validate", "mark", "--validate-min-zncc", "0.5", "--match", "zncc", "--cumulative"],
                                           "--cumulative"),
                                          (["--validate", "mark", "--partial"], "--validate"),
                                          (["--validate", "mark", "--concurrent", "2"], "--validate"),
                                          (["--validate", "smooth"], "usage"), (["--validate"], "usage"),
                                          (["--validate", "mark", "--validate-step", "17"], "usage"),
                                          (["--validate", "mark", "--validate-step", "0"], "usage"),
                                          (["--validate", "mark", "--validate-min-neighbours", "27"], "usage"),
                                          (["--validate", "mark", "--validate-eps", "0"], "usage"),
                                          (["--validate", "mark", "--validate-threshold", "-1"], "usage"),
                                          (["--validate", "mark", "--validate-threshold", "high"], "usage")])
def test_flow3d_validate_argument_errors(tmp_path, extra, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), F32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])   # the status --detrend's counterparts use
    assert needle in run.stdout and "usage" in run.stdout
    assert "[--validate mark|replace [--validate-step S]" in run.stdout
    assert "[--detrend translation|rigid|affine [--detrend-min-zncc T]]" in run.stdout         # the earlier usage text is all still there
    assert not any("validated" in n or "flow-" in n for n in os.listdir(tmp_path))
