"""Principal strains and the polar decomposition of a stored gradient on the GPU: f3d_principal_from_gradient and
f3d_polar_from_gradient against their numpy restatement (tests/from_gradient_ref.py) bit for bit with every statistic, theta_sum
included, in NaN-poisoned containers larger than the box; the group selection and the refusals; the identity with
f3d_principal_strain / f3d_polar_decomposition on the central-difference gradient; window_principal / window_rotation against the
restatement of the window's gradient; the driver's OpticalFlow.window_principal / window_rotation against the free functions; and
bin/flow3d --window-principal / --window-rotation against the binding.

Shapes (w, h, d): every seam of the 64 x 4 x 32 geometry (a wave on 64 x, 4 rows per workgroup, a run of 32 planes) one short, exact
and one over, a second run in z, and the smallest volumes."""
import os
import re
import subprocess

import numpy as np
import pytest

from from_gradient_ref import (GRAD_NAMES, central_gradient, polar_from_gradient_ref, polar_stats, principal_from_gradient_ref,
                               principal_stats)
from polar_ref import NAMES as POLAR_NAMES
from principal_ref import NAMES as PRINCIPAL_NAMES
from strain_ref import same_bits
from window_strain_ref import window_gradient

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
KW = dict(warp_levels_count=8, outer_iterations_count=6, inner_iterations_count=5)
SENTINEL = 0x7F      # byte fill of the outputs: 0x7F7F7F7F = 3.39e38
F32 = np.float32
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 1, 1), (63, 3, 31), (64, 4, 32), (65, 5, 33), (130, 9, 70)]
KINDS = {
    "principal": dict(names=PRINCIPAL_NAMES, group_of=(1, 1, 1, 2, 4, 4, 4, 8, 8, 8), all=15),
    "polar": dict(names=POLAR_NAMES, group_of=(1, 2, 2, 2, 4, 4, 4), all=7),
}


def rotation(angle, axis):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


# the gradients a voxel can be given by name: each a 3 x 3 float64 array (rounded to float32 on the way in)
HALF_TURN = np.diag([-1.0, -1.0, 1.0]) - np.eye(3)
FOLDED = np.diag([-2.0, 0.0, 0.0])
SPECIAL = [rotation(1e-4, (1, 2, 3)) - np.eye(3), rotation(1.0, (3, -1, 2)) - np.eye(3), rotation(3.1, (0, 1, 1)) - np.eye(3), HALF_TURN,
           FOLDED, np.full((3, 3), 1e-41), np.diag([1e-39, -1e-40, 3e-45]),
           np.array([[np.inf, 0.01, 0.02], [0.03, 0.04, 0.05], [0.06, 0.07, 0.08]]),
           np.array([[0.01, -np.inf, 0.02], [0.03, 0.04, 0.05], [0.06, 0.07, 0.08]]),
           np.array([[1e18, 0.01, 0.02], [0.03, 0.04, 0.05], [0.06, 0.07, 0.08]]),
           np.array([[0.01, 0.02, 0.03], [0.04, 0.05, 1e18], [-1e18, 0.07, 0.08]]), np.full((3, 3), 1e18)]


def gradient(case, dims, rng):
    """the nine float32 [z, y, x] arrays of a named input"""
    w, h, d = dims
    shape = (d, h, w)
    n = d * h * w
    if case == "zero":
        return [np.zeros(shape, F32) for _ in range(9)]
    if case == "tenth":                                   # 0.1 I: three equal eigenvalues
        return [np.full(shape, 0.1 if k in (0, 4, 8) else 0.0, F32) for k in range(9)]
    if case == "diagonal":                                # no off-diagonal anywhere: the sweeps' ballot lets every wave go at once
        return [rng.normal(0, 0.05, shape).astype(F32) if k in (0, 4, 8) else np.zeros(shape, F32) for k in range(9)]
    g = [rng.normal(0, 0.05, n).astype(F32) for _ in range(9)]
    if case == "nan":                                     # every third voxel has exactly one entry NaN, each entry in turn
        for i in range(0, n, 3):
            g[(i // 3) % 9][i] = np.nan
    elif case == "special":                               # every other voxel is one of the named gradients, each in turn
        for i in range(0, n, 2):
            s = SPECIAL[(i // 2) % len(SPECIAL)]
            for k in range(9):
                with np.errstate(over="ignore"):
                    g[k][i] = F32(s[k // 3, k % 3])
    else:
        assert case == "random"
    return [a.reshape(shape) for a in g]


def reference(kind, grad):
    """(fields, stats) of the restatement"""
    if kind == "principal":
        f = principal_from_gradient_ref(grad)
        return f, principal_stats(f)
    f, folded = polar_from_gradient_ref(grad)
    return f, polar_stats(f, folded)


def in_a_larger_container(f3d, kind, grad, mask=None, stats=True, null_unselected=True, shared=False):
    """the entry on a box in the corner of NaN-poisoned containers three columns, two rows and a plane larger: the whole output
    containers (sentinel-filled before the call) and the statistics.  shared: entries whose arrays are the same object share a container."""
    K = KINDS[kind]
    mask = K["all"] if mask is None else mask
    d, h, w = grad[0].shape
    cdims = (w + 3, h + 2, d + 1)
    fn = f3d._principal_from_gradient_entry() if kind == "principal" else f3d._polar_from_gradient_entry()
    box = f3d.Containers(*cdims)
    try:
        ins, seen = [], {}
        for a in grad:
            if shared and id(a) in seen:
                ins.append(seen[id(a)])
                continue
            ins.append(box.new(a))
            seen[id(a)] = ins[-1]
        outs = [box.alloc(fill=SENTINEL) for _ in K["names"]]
        box.set_current()
        arr = [p if (mask & g or not null_unselected) else 0 for p, g in zip(outs, K["group_of"])]
        st = (f3d.PrincipalStats() if kind == "principal" else f3d.PolarStats()) if stats else None
        f3d.check(fn((f3d._dp * 9)(*ins), (f3d._dp * len(arr))(*arr), mask, w, h, d, st), "from gradient")
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


def check_stats(got, want, what=""):
    """every statistic by value: the counts, the float32 extremes, the double sum to the last bit"""
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (what, k, got[k], want[k])


def check_fields(got, want, names, what=""):
    for n in names:
        assert same_bits(got[n], want[n]), (what, n)


# ---- the kernels against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["random", "nan", "zero", "tenth", "diagonal", "special"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_entries_equal_the_restatement_bit_for_bit(f3d, dims, case):
    rng = np.random.default_rng(dims[0] * 7919 + dims[1] * 31 + dims[2])
    grad = gradient(case, dims, rng)
    total = dims[0] * dims[1] * dims[2]
    for kind, K in KINDS.items():
        want, want_stats = reference(kind, grad)
        full, st = in_a_larger_container(f3d, kind, grad)
        for name, got in zip(K["names"], full):
            check_box(got, want[name], dims, f"{kind} {dims} {case} {name}")
        check_stats(st, want_stats, f"{kind} {dims} {case}")
        if case == "nan":
            assert st["defined"] + st.get("folded", 0) == total - len(range(0, total, 3))
        elif case != "special":
            assert st["defined"] == total
        if case == "zero":
            assert all((full[i][:dims[2], :dims[1], :dims[0]] == 0).all() for i in range(4)) if kind == "principal" else \
                st["theta_max"] == 0 and st["l1_max"] == 1 and st["l3_min"] == 1 and st["theta_sum"] == 0
        if case == "tenth" and kind == "principal":
            assert st["shear_max"] == 0 and st["e1_max"] == st["e3_min"]
        if dims == (65, 5, 33):                           # a second call gives the same bits
            again, st2 = in_a_larger_container(f3d, kind, grad)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(full, again))
            check_stats(st2, st)


def test_the_named_gradients_give_what_their_names_say(f3d):
    """one voxel each, in SPECIAL's order, along x: the rotations come back as their angles, the exact half turn as theta = pi with a
    zero vector, G00 = -2 as folded, the denormals as no deformation"""
    n = len(SPECIAL)
    with np.errstate(over="ignore"):
        grad = [np.array([s[k // 3, k % 3] for s in SPECIAL], np.float64).astype(F32).reshape(1, 1, n) for k in range(9)]
    want, folded = polar_from_gradient_ref(grad)
    full, st = in_a_larger_container(f3d, "polar", grad)
    got = {name: a[:1, :1, :n] for name, a in zip(POLAR_NAMES, full)}
    check_fields(got, want, POLAR_NAMES)
    check_stats(st, polar_stats(want, folded))
    theta = got["theta"][0, 0]
    # the nine float32 entries of R - I are each off by at most 2^-24 * 2 = 1.2e-7, which turns R by at most their Frobenius norm,
    # 3.6e-7; some 100 float32 operations of 6e-8 each follow: 1e-5 covers both
    for i, angle in enumerate((1e-4, 1.0, 3.1)):
        assert abs(float(theta[i]) - angle) < 1e-5, (i, theta[i])
    assert theta[3].view(np.uint32) == 0x40490FDB and all(got[c][0, 0, 3] == 0 for c in ("rx", "ry", "rz"))
    assert all(got[c][0, 0, 3] == 1 for c in ("l1", "l2", "l3"))
    assert all(np.isnan(got[c][0, 0, 4]) for c in POLAR_NAMES) and folded[0, 0, 4] and st["folded"] >= 1
    for i in (5, 6):                                      # denormals are kept, and deform nothing
        assert theta[i] < 1e-30 and got["l1"][0, 0, i] == 1 and got["l3"][0, 0, i] == 1
    wantp = principal_from_gradient_ref(grad)
    full, st = in_a_larger_container(f3d, "principal", grad)
    gotp = {name: a[:1, :1, :n] for name, a in zip(PRINCIPAL_NAMES, full)}
    check_fields(gotp, wantp, PRINCIPAL_NAMES)
    check_stats(st, principal_stats(wantp))
    # rotations do not strain: E of the rounded R is off by the same 1.2e-7 per entry of F, twice per product, three products per entry
    assert all(abs(float(gotp["e1"][0, 0, i])) < 5e-6 and abs(float(gotp["e3"][0, 0, i])) < 5e-6 for i in (0, 1, 2, 3))
    assert gotp["e1"][0, 0, 4] == 0 and gotp["e3"][0, 0, 4] == 0                                   # E of diag(-2, 0, 0) is 0: E is blind to the fold


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_group_writes_exactly_its_outputs(f3d, kind):
    K = KINDS[kind]
    dims = (65, 5, 33)
    grad = gradient("nan", dims, np.random.default_rng(11))
    want, want_stats = reference(kind, grad)
    singles = [1 << b for b in range(4 if kind == "principal" else 3)]
    for mask in singles + [K["all"]]:
        for stats, null_unselected in ((False, False), (True, True)):
            full, st = in_a_larger_container(f3d, kind, grad, mask, stats, null_unselected)
            for name, group, got in zip(K["names"], K["group_of"], full):
                check_box(got, want[name] if mask & group else None, dims, f"{kind} mask {mask} stats {stats} {name}")
            if stats:
                check_stats(st, want_stats, f"{kind} mask {mask}")     # the statistics do not depend on what is stored


def test_two_entries_may_be_the_same_container(f3d):
    dims = (65, 5, 33)
    a, b, c = (np.random.default_rng(4).normal(0, 0.05, (3,) + dims[::-1]).astype(F32))
    grad = [a, b, c, b, a, b, c, b, a]
    for kind, K in KINDS.items():
        want, want_stats = reference(kind, grad)
        full, st = in_a_larger_container(f3d, kind, grad, shared=True)
        for name, got in zip(K["names"], full):
            check_box(got, want[name], dims, f"{kind} shared {name}")
        check_stats(st, want_stats)


def test_statistics_of_volumes_with_nothing_defined(f3d):
    nan = np.full((3, 4, 5), np.nan, F32)
    zero = np.zeros((3, 4, 5), F32)
    grad = [zero] * 8 + [nan]
    st = f3d.principal_from_gradient(grad)["stats"]
    assert st["defined"] == 0 and all(np.isnan(st[k]) for k in ("e1_max", "e3_min", "shear_max"))
    got = f3d.polar_from_gradient(grad)
    st = got["stats"]
    assert st["defined"] == 0 and st["folded"] == 0 and st["theta_sum"] == 0.0
    assert all(np.isnan(st[k]) for k in ("theta_max", "l1_max", "l3_min"))
    assert set(got) == set(POLAR_NAMES) | {"stats"} and all(np.isnan(got[n]).all() for n in POLAR_NAMES)


# ---- the same bits as the stencil kernels ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def holed():
    """a displacement on (65, 5, 33) with strains of a few percent, a rotation, and 6 % of its samples missing"""
    w, h, d = 65, 5, 33
    rng = np.random.default_rng(21)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    comps = []
    for c in range(3):
        a = 0.8 * np.sin(0.11 * x + 0.3 * c) * np.cos(0.07 * y) + 0.05 * z - 0.03 * x * (c == 1) + 0.02 * rng.standard_normal((d, h, w))
        a = a.astype(F32)
        a[rng.random((d, h, w)) < 0.02] = np.nan
        comps.append(a)
    return comps


def test_the_central_gradient_gives_the_stencil_kernels_bits(f3d, holed):
    grad = central_gradient(*holed)
    old = f3d.principal_strain(*holed, fields=("val", "shear", "dir1", "dir3"))
    new = f3d.principal_from_gradient(grad, fields=("val", "shear", "dir1", "dir3"))
    check_fields(new, old, PRINCIPAL_NAMES, "principal")
    check_stats(new["stats"], old["stats"], "principal")
    assert 0 < old["stats"]["defined"] < holed[0].size
    old = f3d.polar_decomposition(*holed)
    new = f3d.polar_from_gradient(grad)
    check_fields(new, old, POLAR_NAMES, "polar")
    check_stats(new["stats"], old["stats"], "polar")                  # theta_sum to the last bit: the same order of reduction
    assert old["stats"]["theta_sum"] > 0
    new = f3d.polar_from_gradient(dict(zip(GRAD_NAMES, grad)), fields="stretch")       # ROT = false, by name from a dict
    check_fields(new, old, ("l1", "l2", "l3"), "stretch alone")
    assert set(new) == {"l1", "l2", "l3", "stats"}
    check_stats(new["stats"], old["stats"], "stretch alone")


# ---- from the displacement to the fields of the window's gradient ----------------------------------------------------------------------------

@pytest.mark.parametrize("r", (1, 2, 3))
def test_window_principal_and_rotation_equal_the_restatement_of_the_window_gradient(f3d, r):
    w, h, d = 37, 23, 11
    rng = np.random.default_rng(100 + r)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    comps = []
    for c in range(3):
        a = (0.8 * np.sin(0.11 * x + 0.3 * c) * np.cos(0.07 * y) + 0.05 * z + 0.02 * rng.standard_normal((d, h, w))).astype(F32)
        a[rng.random((d, h, w)) < 0.03] = np.nan
        comps.append(a)
    G, _, fitted = window_gradient(*comps, r)
    grad = [np.where(fitted, G[c][a], F32(np.nan)).astype(F32) for c in range(3) for a in range(3)]
    stored = f3d.window_strain(*comps, radius=r, fields=("vol", "grad"))
    assert all(same_bits(stored[n], g) for n, g in zip(GRAD_NAMES, grad))

    want, want_stats = reference("principal", grad)
    everything = ("val", "shear", "dir1", "dir3")
    for got in (f3d.window_principal(*comps, radius=r, fields=everything), f3d.principal_from_gradient(stored, fields=everything),
                f3d.principal_from_gradient([stored[n] for n in GRAD_NAMES], fields=everything)):
        check_fields(got, want, PRINCIPAL_NAMES, f"principal r={r}")
        check_stats(got["stats"], want_stats, f"principal r={r}")
    want, want_stats = reference("polar", grad)
    for got in (f3d.window_rotation(*comps, radius=r), f3d.polar_from_gradient(stored)):
        check_fields(got, want, POLAR_NAMES, f"polar r={r}")
        check_stats(got["stats"], want_stats, f"polar r={r}")
    assert 0 < want_stats["defined"] < w * h * d
    few = f3d.window_principal(*comps, radius=r, min_count=(2 * r + 1) ** 3)     # min_count reaches the window pass
    assert few["stats"]["defined"] < want_stats["defined"] and set(few) == {"e1", "e2", "e3", "gmax", "stats"}


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
def test_refusals(f3d, kind):
    K = KINDS[kind]
    ALL, count = K["all"], len(K["names"])
    who = b"f3d_principal_from_gradient" if kind == "principal" else b"f3d_polar_from_gradient"
    hip = f3d.hip()
    fn = f3d._principal_from_gradient_entry() if kind == "principal" else f3d._polar_from_gradient_entry()
    box = f3d.Containers(8, 8, 8)
    try:
        grad = [box.new(np.zeros((8, 8, 8), F32)) for _ in range(9)]
        outs = [box.alloc(fill=SENTINEL) for _ in range(count)]
        box.set_current()

        def call(g, o, mask, dims=(8, 8, 8)):
            return fn((f3d._dp * 9)(*g) if g is not None else None, (f3d._dp * count)(*o) if o is not None else None, mask, *dims, None)

        def swapped(seq, i, p):
            s = list(seq)
            s[i] = p
            return s

        bad = [((None, outs, ALL), {})]                                                  # no gradient array
        bad += [((swapped(grad, k, 0), outs, ALL), {}) for k in range(9)]                # a null entry of it
        bad += [
            ((grad, None, ALL), {}),                                                     # no output array
            ((grad, swapped(outs, 0, 0), 1), {}),                                        # null selected outputs
            ((grad, swapped(outs, count - 1, 0), ALL), {}),
            ((grad, outs, 0), {}),                                                       # nothing selected
            ((grad, outs, ALL + 1), {}),                                                 # unknown bit
            ((grad, swapped(outs, 0, outs[1]), ALL), {}),                                # two equal selected outputs
            ((grad, outs, ALL), {"dims": (0, 8, 8)}),                                    # empty, and larger than the container
            ((grad, outs, ALL), {"dims": (8, 8, 9)}),
            ((grad, outs, ALL), {"dims": (9, 8, 8)}),
        ]
        bad += [((grad, swapped(outs, k % count, grad[k]), ALL), {}) for k in range(9)]  # a selected output that is any of the nine inputs
        for args, kw in bad:
            assert call(*args, **kw) == 1, (args[-1], kw)
            assert who in hip.f3d_last_error(), hip.f3d_last_error()
        f3d.sync()
        for p in outs:                                                                   # a refused call writes nothing
            assert (box.download(p, (8, 8, 8)).view(np.uint32) == 0x7F7F7F7F).all()
        # an input or a shared container as an UNSELECTED output is fine
        assert call(grad, swapped(outs, count - 1, grad[3]), 1) == 0
        assert call(grad, swapped(outs, count - 1, outs[0]), 1) == 0
        f3d.sync()
    finally:
        box.free()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def solved(f3d):
    """the flow of the synthetic 48 x 40 x 24 pair and the trajectory of that one pair, with the driver's window fields of both"""
    w, h, d = 48, 40, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    flow = f3d.OpticalFlow()
    flow.initialize(w, h, d)
    out = {}
    try:
        flow.upload(f0, f1)
        flow.compute_resident(silent=True, **KW)
        uvw = flow.download()
        flow.trajectory_begin()
        flow.trajectory_append()
        out["trajectory"] = flow.trajectory_download()[:3]
        before = flow.window_strain(radius=1, fields=("vol", "grad"))
        out["principal"] = flow.window_principal(radius=3, fields=("val", "shear", "dir1", "dir3"))     # needs no window_strain at its radius
        out["rotation"] = flow.window_rotation()
        out["principal_default"] = flow.window_principal()
        out["principal_trajectory"] = flow.window_principal(source="trajectory", radius=1, min_count=27)
        out["rotation_trajectory"] = flow.window_rotation(source="trajectory", radius=2, fields="stretch")
        after = flow.window_strain(radius=1, fields=("vol", "grad"))
        out["window_strain"] = (before, after)
        assert all(np.array_equal(p, q) for p, q in zip(flow.download(), uvw))
        flow.window_principal_end()
        out["rotation_after_principal_end"] = flow.window_rotation()                                   # the gradient's containers come back
        flow.window_rotation_end()
        flow.window_rotation_end()                                                                     # ending twice is harmless
        out["principal_again"] = flow.window_principal(radius=3, fields=("val", "shear", "dir1", "dir3"))
        flow.window_strain_end()
    finally:
        flow.destroy()
    return (w, h, d), (f0, f1), uvw, out


def same_result(got, want, names):
    assert set(got) == set(want)
    for n in want:
        if n != "stats":
            assert same_bits(got[n], want[n]), n
    check_stats(got["stats"], want["stats"])
    assert [n for n in names if n in got] == [n for n in got if n != "stats"]


def test_the_driver_equals_the_free_functions(f3d, solved):
    dims, _, uvw, out = solved
    everything = ("val", "shear", "dir1", "dir3")
    same_result(out["principal"], f3d.window_principal(*uvw, radius=3, fields=everything), PRINCIPAL_NAMES)
    same_result(out["principal_again"], out["principal"], PRINCIPAL_NAMES)
    same_result(out["rotation"], f3d.window_rotation(*uvw), POLAR_NAMES)
    same_result(out["rotation_after_principal_end"], out["rotation"], POLAR_NAMES)
    same_result(out["principal_default"], f3d.window_principal(*uvw), PRINCIPAL_NAMES)
    assert set(out["principal_default"]) == {"e1", "e2", "e3", "gmax", "stats"}
    t = out["trajectory"]
    same_result(out["principal_trajectory"], f3d.window_principal(*t, radius=1, min_count=27), PRINCIPAL_NAMES)
    same_result(out["rotation_trajectory"], f3d.window_rotation(*t, radius=2, fields="stretch"), POLAR_NAMES)
    assert out["principal"]["stats"]["defined"] > 0.9 * dims[0] * dims[1] * dims[2]
    before, after = out["window_strain"]
    same_result(after, before, ("vol",) + GRAD_NAMES)


# ---- bin/flow3d --window-principal / --window-rotation ------------------------------------------------------------------------------------------

P_LINE = re.compile(r"window principal \(r=(\d+)\) frame (\d+) -> frame (\d+): e1 max (\S+), e3 min (\S+), shear max (\S+), (\d+) undefined of "
                    r"(\d+) voxels")
R_LINE = re.compile(r"window rotation \(r=(\d+)\) frame (\d+) -> frame (\d+): angle max (\S+) rad, mean (\S+) rad, stretch max (\S+), min (\S+), "
                    r"(\d+) folded, (\d+) undefined of (\d+) voxels")


def test_cli_equals_the_binding_and_leaves_the_other_options_alone(f3d, tmp_path):
    w, h, d = 40, 36, 24
    f0, f1 = f3d.synth_pair(w, h, d)
    frames = [f0, f1, np.roll(f1, 1, axis=2)]
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / f"f{i}.raw")
        np.ascontiguousarray(f, dtype=F32).tofile(p)
        paths.append(p)
    base = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", str(KW["warp_levels_count"]),
            "--outer", str(KW["outer_iterations_count"]), "--inner", str(KW["inner_iterations_count"]), "--silent", "--frames", *paths]
    others = ["--cumulative", "--strain", "vol,eq", "--window-strain", "vol,grad", "--window-radius", "1", "--principal", "val,dir3",
              "--rotation", "angle,stretch"]
    os.mkdir(tmp_path / "a")
    os.mkdir(tmp_path / "b")
    plain = subprocess.run(base + ["--out", str(tmp_path / "a" / "s")] + others, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    new = ["--window-principal", "val,shear,dir1,dir3", "--window-rotation", "angle,vector,stretch"]
    run = subprocess.run(base + ["--out", str(tmp_path / "b" / "s")] + others + new, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]

    # the files and lines of every other option are the same bytes with and without the new options
    was, now = sorted(os.listdir(tmp_path / "a")), sorted(os.listdir(tmp_path / "b"))
    added = [n for n in now if n not in was]
    assert was and [n for n in now if n in was] == was and all("_wprincipal-" in n or "_wrotation-" in n for n in added)
    for n in was:
        assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read(), n
    theirs = re.compile(r"(strain|window strain|principal|rotation) .*frame \d+ -> frame \d+: ")
    lines = [ln for ln in plain.stdout.splitlines() if theirs.match(ln)]
    assert len(lines) == 2 * 4 and lines == [ln for ln in run.stdout.splitlines() if theirs.match(ln)]

    # and the new files are the binding's fields of the displacement frame 0 -> frame k + 1 that --cumulative wrote
    suffix = f"-{w}-{h}-{d}.raw"
    p_lines, r_lines = P_LINE.findall(run.stdout), R_LINE.findall(run.stdout)
    assert len(p_lines) == len(r_lines) == 2
    assert len(added) == 2 * (10 + 7)
    for k in range(2):
        tag = str(tmp_path / "b" / f"s_{k}")
        disp = [np.fromfile(f"{tag}_disp-{c}{suffix}", F32).reshape(d, h, w) for c in "uvw"]
        want = f3d.window_principal(*disp, radius=1, fields=("val", "shear", "dir1", "dir3"))
        for n in PRINCIPAL_NAMES:
            assert same_bits(np.fromfile(f"{tag}_wprincipal-{n}{suffix}", F32).reshape(d, h, w), want[n]), (k, n)
        m, st = p_lines[k], want["stats"]
        assert (int(m[0]), int(m[1]), int(m[2])) == (1, 0, k + 1) and int(m[7]) == w * h * d and int(m[6]) == w * h * d - st["defined"]
        for txt, val in ((m[3], st["e1_max"]), (m[4], st["e3_min"]), (m[5], st["shear_max"])):
            assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)
        want = f3d.window_rotation(*disp, radius=1)
        for n in POLAR_NAMES:
            assert same_bits(np.fromfile(f"{tag}_wrotation-{n}{suffix}", F32).reshape(d, h, w), want[n]), (k, n)
        m, st = r_lines[k], want["stats"]
        assert (int(m[0]), int(m[1]), int(m[2])) == (1, 0, k + 1) and int(m[9]) == w * h * d
        assert int(m[7]) == st["folded"] and int(m[8]) == w * h * d - st["defined"] - st["folded"]
        for txt, val in ((m[3], st["theta_max"]), (m[4], st["theta_sum"] / st["defined"]), (m[5], st["l1_max"]), (m[6], st["l3_min"])):
            assert float(txt) == pytest.approx(val, rel=1e-5, abs=1e-12), (txt, val)


def test_cli_each_new_option_works_on_its_own(f3d, tmp_path):
    w, h, d = 24, 20, 16
    f0, f1 = f3d.synth_pair(w, h, d)
    paths = []
    for i, f in enumerate((f0, f1)):
        p = str(tmp_path / f"f{i}.raw")
        np.ascontiguousarray(f, dtype=F32).tofile(p)
        paths.append(p)
    base = [EXE, "--dims", str(w), str(h), str(d), "--f32", "--levels", "4", "--outer", "3", "--inner", "3", "--silent", "--frames", *paths]
    suffix = f"-{w}-{h}-{d}.raw"
    for option, value, tag, names, line in (("--window-principal", "shear", "wprincipal", ("gmax",), P_LINE),
                                            ("--window-rotation", "vector", "wrotation", ("rx", "ry", "rz"), R_LINE)):
        out = tmp_path / tag
        os.mkdir(out)
        run = subprocess.run(base + ["--out", str(out / "o"), option, value, "--window-min-count", "20"], capture_output=True, text=True,
                             timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        flow = [np.fromfile(str(out / f"o_flow-{c}{suffix}"), F32).reshape(d, h, w) for c in "uvw"]
        fn = f3d.window_principal if tag == "wprincipal" else f3d.window_rotation
        want = fn(*flow, radius=2, min_count=20, fields=value)
        made = sorted(n for n in os.listdir(out) if f"_{tag}-" in n)
        assert made == sorted(f"o_{tag}-{n}{suffix}" for n in names)
        for n in names:
            assert same_bits(np.fromfile(str(out / f"o_{tag}-{n}{suffix}"), F32).reshape(d, h, w), want[n]), n
        found = line.findall(run.stdout)
        assert len(found) == 1 and (int(found[0][0]), int(found[0][1]), int(found[0][2])) == (2, 0, 1)
        assert not any("wstrain" in n or "_principal-" in n or "_rotation-" in n for n in os.listdir(out))
