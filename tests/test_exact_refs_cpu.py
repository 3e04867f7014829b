"""The independent references of tests/exact_ref.py without a GPU: the exact constructions prove themselves exact and give the
closed forms, the float64 header strain is np.gradient's where there are no holes, and the float32 restatements that the GPU tests
match bit for bit (tests/strain_ref.py, tests/trajectory_ref.py) agree with all of them -- so a rule that kernel and restatement
misread together is caught here."""
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
from strain_ref import NAMES, gradient_ref, strain_ref, strain_stats_ref
from trajectory_ref import compose_sequence_ref, same_bits

F32 = np.float32


def check_strain_against_header(got, comps, label=""):
    """float32 outputs (dict) of the displacement comps against the float64 header strain: the same NaN set, and values within the
    rounding bound of exact_ref.strain_tolerance"""
    G, und = X.gradient64(*comps)
    want = X.strain64(G, und)
    tol = X.strain_tolerance(G)
    for n in NAMES:
        assert np.array_equal(np.isnan(got[n]), und), f"{label} {n}: undefined set"
    ok = ~und
    assert np.all(np.abs(got["vol"][ok] - want["vol"][ok]) <= tol["vol"][ok]), f"{label} vol"
    for n in NAMES[1:7]:
        assert np.all(np.abs(got[n][ok] - want[n][ok]) <= tol["e"][ok]), f"{label} {n}"
    eq2 = got["eq"][ok].astype(np.float64) ** 2
    assert np.all(np.abs(eq2 - want["eq"][ok] ** 2) <= tol["eq2"][ok]), f"{label} eq"


# ---- exact strain -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(X.STRAIN_AFFINE)))
def test_affine_strain_is_exact_in_the_header_order(k):
    A, _ = X.STRAIN_AFFINE[k]
    exact = X.header_fields_exact(A)                 # asserts every float32 operation exact
    cf = X.closed_form_fraction(A)
    for n in NAMES[:7]:
        assert Fraction(exact[n]) == cf[n], n
    # the restatement's float32 arithmetic on the same constant gradient gives the same numbers
    G = [[np.full((1, 1, 1), A[r][c], F32) for c in range(3)] for r in range(3)]
    from strain_ref import fields_of_gradient
    f32 = fields_of_gradient(G)
    for n in NAMES[:7]:
        assert float(f32[n][0, 0, 0]) == exact[n], n
    assert X.ulps_apart(f32["eq"][0, 0, 0], X.eq_of_E({n: float(cf[n]) for n in NAMES[1:7]})) <= X.EQ_ULPS


@pytest.mark.parametrize("dims", [(37, 23, 11), (66, 5, 34), (1, 9, 7), (6, 1, 1)])
def test_affine_displacement_with_holes_gives_the_closed_form_where_defined(dims):
    rng = np.random.default_rng(sum(dims))
    for A, b in X.STRAIN_AFFINE:
        comps = X.affine_field(A, b, dims)
        all_nan, one_nan = X.seam_holes(dims, rng, density=0.05)
        comps = X.with_holes(comps, all_nan, one_nan, which=2)
        und = X.predicted_undefined(all_nan | one_nan)
        assert und.any() and (~und).any()
        out = strain_ref(*comps)
        # exact where defined: faces and rims take one-sided differences of an affine field, which are exact as well
        cf = X.closed_form_fraction(A)
        eq = X.eq_of_E({n: float(cf[n]) for n in NAMES[1:7]})
        # an axis of size one has a zero column: the closed form of A with that column cleared
        A0 = [[0.0 if (dims[c] == 1) else A[r][c] for c in range(3)] for r in range(3)]
        cf0 = X.closed_form_fraction(A0)
        eq0 = X.eq_of_E({n: float(cf0[n]) for n in NAMES[1:7]})
        for n in NAMES:
            assert np.array_equal(np.isnan(out[n]), und), n
        for n in NAMES[:7]:
            assert (out[n][~und] == F32(float(cf0[n]))).all() and float(F32(float(cf0[n]))) == cf0[n], n
        assert (X.ulps_apart(out["eq"][~und], eq0) <= X.EQ_ULPS).all()
        if all(n > 1 for n in dims):
            assert cf0 == cf and eq0 == eq


def test_predicted_undefined_set_follows_the_hole_geometry():
    """undefined = missing, or isolated along one axis (holes at x - 1 and x + 1, or a face and a hole); a size-one axis isolates
    nothing"""
    miss = np.zeros((5, 6, 7), bool)
    miss[2, 3, 2] = miss[2, 3, 4] = True
    want = miss.copy()
    want[2, 3, 3] = True
    assert np.array_equal(X.predicted_undefined(miss), want)
    miss = np.zeros((5, 6, 7), bool)
    miss[2, 3, 1] = miss[0, 4, 5] = True
    want = miss.copy()
    want[2, 3, 0] = True               # the x = 0 face below, a hole above
    want[0, 5, 5] = True               # a hole below, the y = H - 1 face above
    want[0, 4, 6] = True               # a hole below, the x = W - 1 face above
    assert np.array_equal(X.predicted_undefined(miss), want)
    miss3 = np.zeros((3, 1, 4), bool)
    miss3[:, 0, 1] = True
    und3 = X.predicted_undefined(miss3)
    assert und3[:, 0, 0].all() and not und3[:, 0, 2:].any()


# ---- the float64 header strain --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(17, 13, 9), (2, 5, 3), (1, 8, 6), (9, 1, 1)])
def test_masked_stencil_is_np_gradient_without_holes(dims):
    comps = X.smooth_displacement(dims, "quadratic", seed=3)
    G, und = X.gradient64(*comps)
    Gn = X.gradient_np(*comps)
    assert not und.any()
    for r in range(3):
        for c in range(3):
            assert np.allclose(G[r][c], Gn[r][c], rtol=0, atol=1e-12), (r, c)


@pytest.mark.parametrize("kind", ["quadratic", "sine"])
@pytest.mark.parametrize("dims", [(33, 17, 9), (65, 4, 3), (1, 12, 10), (8, 1, 5), (5, 6, 1)])
def test_restatement_agrees_with_the_float64_header(kind, dims):
    comps = X.smooth_displacement(dims, kind, seed=sum(dims))
    check_strain_against_header(strain_ref(*comps), comps, "no holes")
    rng = np.random.default_rng(7)
    holed = X.with_holes(comps, *X.seam_holes(dims, rng, density=0.04))
    check_strain_against_header(strain_ref(*holed), holed, "holes")


def test_the_tolerance_sees_a_wrong_side_and_a_wrong_neighbour():
    """the float64 check has teeth: the restatement with a face rule taken from the wrong side, or with the x + 2 neighbour, fails it"""
    dims = (24, 10, 8)
    comps = X.smooth_displacement(dims, "quadratic", seed=11)
    G, und = X.gradient64(*comps)
    want = X.strain64(G, und)
    tol = X.strain_tolerance(G)
    Gr, _ = gradient_ref(*comps)
    from strain_ref import fields_of_gradient
    for mutate in ("wrong side", "x + 2"):
        Gm = [[np.array(Gr[r][c]) for c in range(3)] for r in range(3)]
        u = comps[0]
        if mutate == "wrong side":       # the x = 0 face takes the difference one voxel further in
            Gm[0][0][:, :, 0] = u[:, :, 2] - u[:, :, 1]
        else:
            Gm[0][0][:, :, 1:-2] = (u[:, :, 3:] - u[:, :, :-3]) * F32(0.5)
        bad = fields_of_gradient(Gm)
        assert np.any(np.abs(bad["vol"] - want["vol"]) > tol["vol"]), mutate


# ---- exact composition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,steps", [((37, 23, 11), 3), ((129, 5, 65), 3), ((65, 5, 2), 3), ((1, 1, 1), 3), ((3, 1, 7), 3),
                                        ((1024, 1024, 1025), 2)])
def test_affine_composition_is_exact(dims, steps):
    assert X.prove_compose_exact(X.COMPOSE_AFFINE[:steps], dims)
    if steps < len(X.COMPOSE_AFFINE):       # the proof has teeth: one step more is not exact at this size
        with pytest.raises(AssertionError, match="not exact"):
            X.prove_compose_exact(X.COMPOSE_AFFINE[:steps + 1], dims)


@pytest.mark.parametrize("dims", [(37, 23, 11), (64, 4, 33), (65, 5, 2), (3, 1, 7), (1, 1, 1)])
def test_restatement_composes_affine_flows_to_the_exact_map(dims):
    """three steps from zero: the restatement equals the exact composed map bit for bit, and a point is lost exactly when its exact
    position leaves [0, n-1] at some step"""
    flows = [X.affine_field(A, b, dims) for A, b in X.COMPOSE_AFFINE]
    got = compose_sequence_ref(flows)
    want = X.compose_affine_expected(X.COMPOSE_AFFINE, dims)
    for k, (g, e) in enumerate(zip(got, want)):
        for c in range(3):
            assert same_bits(g[c], e[c]), (k, c)
    n = np.prod(dims)
    lost = [int(np.isnan(e[0]).sum()) for e in want]
    assert lost == sorted(lost)
    if min(dims) > 2:
        assert 0 < lost[-1] < n


def test_composition_mid_sequence_matches_in_a_plane_window():
    """the expected map of a plane window is the window of the whole expected map (the chunked check of the big GPU test)"""
    dims = (20, 9, 15)
    whole = X.compose_affine_expected(X.COMPOSE_AFFINE[:2], dims)
    part = X.compose_affine_expected(X.COMPOSE_AFFINE[:2], dims, 4, 11)
    for a, b in zip(whole, part):
        for c in range(3):
            assert same_bits(a[c][4:11], b[c])


# ---- statistics references ------------------------------------------------------------------------------------------------

def test_fsum_is_exact_where_numpy_is_not():
    vals = np.array([1e16, 1.0, -1e16, 1.0] * 1000)
    assert X.fsum(vals) == 2000.0


def test_restatement_statistics_sum_agrees_with_fsum():
    comps = X.smooth_displacement((40, 30, 20), "sine", amp=0.3, seed=1)
    out = strain_ref(*comps)
    st = strain_stats_ref(out["vol"], out["eq"])
    assert abs(st["vol_sum"] - X.fsum(out["vol"].astype(np.float64))) <= 1e-12 * X.fsum(np.abs(out["vol"].astype(np.float64)))


def test_finite_abs_max_contract():
    a = np.array([-3.5, 2.0, np.nan, np.inf, -np.inf, -0.0], F32)
    assert X.finite_abs_max(a) == F32(3.5)
    assert X.finite_abs_max(np.array([np.nan, np.inf], F32)) == 0 and not np.signbit(X.finite_abs_max(np.array([-0.0], F32)))
    den = np.array([1e-45, -3e-42, 2e-40], F32)
    assert X.finite_abs_max(den) == F32(2e-40) and X.finite_abs_max(den) > 0


def test_magnitude_is_the_float32_expression():
    rng = np.random.default_rng(2)
    u, v, w = (rng.uniform(-4, 4, 1000).astype(F32) for _ in range(3))
    m = X.magnitude32(u, v, w)
    assert m.dtype == F32
    assert np.allclose(m, np.sqrt(u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2 + w.astype(np.float64) ** 2), rtol=3e-7)
