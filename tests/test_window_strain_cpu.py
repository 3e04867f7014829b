"""The definition of the strain window (include/f3d.h, f3d_window_strain) checked on its numpy restatement, tests/window_strain_ref.py,
without a device: it reproduces an affine displacement exactly whatever the holes, agrees with a float64 least-squares fit of every
window, reduces to the mean of nine central differences at radius 1, has the textbook noise gain, and follows the rules of the
undefined voxels.  tests/test_gpu_window_strain.py then holds the kernel to the restatement bit for bit."""
import numpy as np
import pytest

import strain_ref
from window_strain_ref import GRAD_NAMES, window_gradient, window_strain_ref

RADII = (1, 2, 3)
# Worst |G - lstsq| of the restatement over LSTSQ_SHAPES x RADII, measured here (DESIGN.md section 19 has the table): 2.98e-9 at
# |G| <= 0.1, which is the rounding of G to float32 (half an ulp is 1.9e-9 below 1/16 and 3.7e-9 above) plus what lstsq itself loses
# on offsets of 150 voxels.  The bound is four times that; it is an absolute bound for gradients of this size.
LSTSQ_WORST = 3.0e-9
LSTSQ_BOUND = 4 * LSTSQ_WORST
LSTSQ_SHAPES = [(13, 10, 9), (70, 12, 1), (66, 1, 5), (1, 7, 6), (5, 1, 1)]


def affine_field(rng, dims):
    w, h, d = dims
    M = rng.integers(-8, 9, (3, 3)) / 16.0
    t = rng.integers(-16, 17, 3) / 8.0
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    comps = [(t[c] + M[c, 0] * x + M[c, 1] * y + M[c, 2] * z).astype(np.float32) for c in range(3)]
    return M, comps


@pytest.mark.parametrize("holes", (0.0, 0.3, 0.6))
@pytest.mark.parametrize("r", RADII)
def test_an_affine_displacement_is_reproduced_exactly_whatever_the_holes(r, holes):
    dims = (13, 10, 9)
    rng = np.random.default_rng(100 + r)
    M, (u, v, w) = affine_field(rng, dims)
    v[rng.random(v.shape) < holes] = np.nan
    G, present, fitted = window_gradient(u, v, w, r, min_count=4)   # four points: the least a plane through three axes needs
    assert fitted.sum() > 0
    worst = max(float(np.abs(G[c][a][fitted].astype(np.float64) - M[c, a]).max()) for c in range(3) for a in range(3))
    thin = int((present & ~fitted).sum())
    print(f"r={r} holes={holes}: max |G - M| {worst}, {thin} thin of {int(present.sum())} present")
    assert worst == 0.0
    if r >= 2:
        assert thin == 0
    elif holes == 0.6:
        assert thin <= 0.05 * present.sum()


def noisy_field(rng, dims, holes):
    w, h, d = dims
    comps = []
    for c in range(3):
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        a = 150.0 * rng.random() + 0.02 * x - 0.015 * y + 0.01 * z + 0.02 * rng.standard_normal((d, h, w))
        comps.append(a.astype(np.float32))
    comps[int(rng.integers(0, 3))][rng.random((d, h, w)) < holes] = np.nan
    return comps


def lstsq_gradient(comps, p, r, present):
    """the float64 least-squares plane through the present samples of the window of voxel p = (z, y, x): 3 x 3 slopes, or None when
    the design matrix (constant + the axes of size > 1) has no full rank"""
    d, h, w = present.shape
    z0, y0, x0 = p
    rows, vals = [], []
    for k in range(max(0, z0 - r), min(d, z0 + r + 1)):
        for j in range(max(0, y0 - r), min(h, y0 + r + 1)):
            for i in range(max(0, x0 - r), min(w, x0 + r + 1)):
                if present[k, j, i]:
                    rows.append((1.0, i - x0, j - y0, k - z0))
                    vals.append([float(c[k, j, i]) for c in comps])
    axes = [a for a, n in enumerate((w, h, d)) if n > 1]
    A = np.array(rows, np.float64)[:, [0] + [1 + a for a in axes]]
    if np.linalg.matrix_rank(A) < A.shape[1]:
        return None
    sol = np.linalg.lstsq(A, np.array(vals, np.float64), rcond=None)[0]
    G = np.zeros((3, 3))
    for col, a in enumerate(axes):
        G[:, a] = sol[1 + col]
    return G


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("dims", LSTSQ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_it_is_the_least_squares_fit_of_the_window(dims, r):
    rng = np.random.default_rng(dims[0] * 131 + dims[1] * 17 + dims[2] + r)
    comps = noisy_field(rng, dims, 0.25 + 0.05 * rng.random())
    G, present, fitted = window_gradient(*comps, r, min_count=1)
    worst, largest, checked = 0.0, 0.0, 0
    for p in zip(*np.nonzero(present)):
        want = lstsq_gradient(comps, p, r, present)
        assert (want is not None) == bool(fitted[p]), (p, "the determinant test and the rank of the window disagree")
        if want is None:
            continue
        got = np.array([[G[c][a][p] for a in range(3)] for c in range(3)], np.float64)
        worst = max(worst, float(np.abs(got - want).max()))
        largest = max(largest, float(np.abs(want).max()))
        checked += 1
    print(f"{dims} r={r}: {checked} voxels, max |G - lstsq| {worst:.3g} at |G| <= {largest:.3g}")
    assert checked > 0 or dims == (5, 1, 1)
    assert worst <= LSTSQ_BOUND


def test_at_radius_1_it_is_the_mean_of_the_nine_central_differences():
    # noise of deviation 0.06: G00 then reaches the 0.06 .. 0.1 at which LSTSQ_BOUND was measured (the rounding of G to float32 grows
    # with G: unit noise gives 2.8e-8 at |G00| near 1)
    rng = np.random.default_rng(5)
    u = (0.06 * rng.standard_normal((9, 10, 11))).astype(np.float32)
    G, present, fitted = window_gradient(u, u, u, 1)
    assert fitted.all()
    u64 = u.astype(np.float64)
    cd = np.zeros_like(u64)
    cd[:, :, 1:-1] = (u64[:, :, 2:] - u64[:, :, :-2]) * 0.5
    mean = np.zeros_like(u64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            mean[1:-1, 1:-1, :] += cd[1 + dz:cd.shape[0] - 1 + dz, 1 + dy:cd.shape[1] - 1 + dy, :]
    mean /= 9.0
    inner = (slice(1, -1),) * 3
    worst = float(np.abs(G[0][0][inner].astype(np.float64) - mean[inner]).max())
    print(f"max |G00 - mean of nine central differences| {worst:.3g} at |G00| <= {float(np.abs(mean[inner]).max()):.3g}")
    assert worst <= LSTSQ_BOUND


def test_the_noise_gain_is_the_textbook_one():
    rng = np.random.default_rng(7)
    comps = [rng.standard_normal((24, 24, 24)).astype(np.float32) for _ in range(3)]
    for r, want in zip(RADII, (0.2357, 0.0632, 0.0270)):
        G, _, fitted = window_gradient(*comps, r)
        inner = (slice(r, -r),) * 3
        assert fitted[inner].all()
        got = float(np.std(np.stack([G[c][a][inner] for c in range(3) for a in range(3)]).astype(np.float64)))
        print(f"r={r}: std of G {got:.4f}, 1 / sqrt((2r+1)^2 sum i^2) = {want:.4f}")
        assert abs(got - want) <= 0.05 * want


def test_the_rules_of_size_one_axes_and_undefined_voxels():
    rng = np.random.default_rng(9)
    # size-1 axes: their columns are zero, the fit runs over the rest
    line = [rng.standard_normal((5, 1, 1)).astype(np.float32) for _ in range(3)]          # (w, h, d) = (1, 1, 5)
    line[1][0, 0, 0] = np.nan
    out, st = window_strain_ref(*line, 1, min_count=4)
    assert st["defined"] == 0 and st["lost"] == 1 and st["thin"] == 4 and np.isnan(out["vol"]).all()
    out, st = window_strain_ref(*line, 3, min_count=4)
    assert st["defined"] == 4 and st["lost"] == 1 and st["thin"] == 0
    ok = ~np.isnan(out["vol"])
    assert ok.sum() == 4 and not ok[0, 0, 0]
    for c in range(3):
        assert (out[f"G{c}0"][ok] == 0).all() and (out[f"G{c}1"][ok] == 0).all() and (out[f"G{c}2"][ok] != 0).all()
    # 2 x 2 x 2 with three present points: every window is a plane
    cube = [rng.standard_normal((2, 2, 2)).astype(np.float32) for _ in range(3)]
    keep = np.zeros((2, 2, 2), bool)
    keep[0, 0, 0] = keep[0, 1, 1] = keep[1, 0, 1] = True
    cube[2][~keep] = np.nan
    out, st = window_strain_ref(*cube, 1, min_count=1)
    assert st["defined"] == 0 and st["lost"] == 5 and st["thin"] == 3
    assert all(np.isnan(out[k]).all() for k in out)
    # min_count above n makes a voxel thin; a NaN centre is lost
    vol = [rng.standard_normal((6, 6, 6)).astype(np.float32) * np.float32(0.01) for _ in range(3)]
    vol[0][3, 3, 3] = np.nan
    out, st = window_strain_ref(*vol, 1, min_count=27)
    assert st["lost"] == 1 and np.isnan(out["vol"][3, 3, 3])
    full = np.zeros((6, 6, 6), bool)
    full[1:-1, 1:-1, 1:-1] = True
    full[2:5, 2:5, 2:5] = False                                  # the windows that hold the hole have 26 points
    assert np.array_equal(~np.isnan(out["vol"]), full)
    assert st["thin"] == 216 - 1 - int(full.sum()) and st["defined"] == int(full.sum())
    out, st = window_strain_ref(*vol, 1, min_count=8)
    assert st["thin"] == 0 and st["defined"] == 215


def test_the_outputs_are_the_strain_expressions_of_the_gradient():
    rng = np.random.default_rng(11)
    comps = [(rng.standard_normal((7, 8, 9)) * 0.3).astype(np.float32) for _ in range(3)]
    comps[2][rng.random((7, 8, 9)) < 0.1] = np.nan
    out, st = window_strain_ref(*comps, 2)
    G = [[out[f"G{c}{a}"] for a in range(3)] for c in range(3)]
    again = strain_ref.fields_of_gradient(G)
    for name in strain_ref.NAMES:
        assert strain_ref.same_bits(out[name], again[name]), name
    assert set(out) == set(strain_ref.NAMES) | set(GRAD_NAMES)
    want = strain_ref.strain_stats_ref(out["vol"], out["eq"])
    for k in want:
        assert st[k] == want[k] or (np.isnan(st[k]) and np.isnan(want[k])), k
