"""Float32 numpy restatement of f3d_principal_from_gradient and f3d_polar_from_gradient (include/f3d.h), the checker of the kernels.

Nothing new is computed here: E comes from strain_ref.fields_of_gradient, rules 2-4 from principal_ref.principal_of_tensor, rules
1-6 from polar_ref.polar_of_gradient, the statistics from the two *_stats_ref functions.  What this file adds is the definition of
the entries: a voxel is undefined iff any of its nine entries is NaN, and that mask is applied AFTER the arithmetic (the kernel
rotates the zero matrix there instead, which no output shows).  A gradient is a sequence of nine arrays in the ABI's order
G00 G01 G02 G10 G11 G12 G20 G21 G22.

The statistics of the kernels fold with fmaxf / fminf from -inf / +inf, which pass over a NaN, and numpy's max does not.  Where
every counted value is a number the two are the same and the existing functions are the whole answer; an infinity or an overflow in
G can leave a NaN in e3, gmax or theta of a counted voxel, and there the fold is restated (theta_sum is then NaN in any order)."""
import numpy as np

from polar_ref import NAMES as POLAR_NAMES, polar_of_gradient, polar_stats_ref
from principal_ref import NAMES as PRINCIPAL_NAMES, principal_of_tensor, principal_stats_ref
from strain_ref import fields_of_gradient, gradient_ref

F32 = np.float32
GRAD_NAMES = ("G00", "G01", "G02", "G10", "G11", "G12", "G20", "G21", "G22")
_E = ("exx", "eyy", "ezz", "exy", "exz", "eyz")


def rows(grad):
    """G[r][c] of the nine arrays in ABI order (or of the dict that names them G00 .. G22)"""
    if isinstance(grad, dict):
        grad = [grad[n] for n in GRAD_NAMES]
    g = [np.asarray(a, dtype=F32) for a in grad]
    assert len(g) == 9
    return [g[0:3], g[3:6], g[6:9]]


def flat(G):
    """the nine arrays in ABI order of G[r][c]"""
    return [G[r][c] for r in range(3) for c in range(3)]


def undefined(grad):
    g = flat(rows(grad))
    out = np.isnan(g[0])
    for a in g[1:]:
        out = out | np.isnan(a)
    return out


def central_gradient(u, v, w):
    """the nine arrays f3d_flow_strain's rules give, NaN at its undefined voxels: what makes the from-gradient entries repeat
    f3d_principal_strain and f3d_polar_decomposition"""
    G, defined = gradient_ref(u, v, w)
    return [np.where(defined, g, F32(np.nan)).astype(F32) for g in flat(G)]


def principal_from_gradient_ref(grad):
    """dict name -> float32 array of all ten outputs (NaN where the voxel is undefined)"""
    G = rows(grad)
    with np.errstate(all="ignore"):
        f = fields_of_gradient(G)
        out = principal_of_tensor(tuple(f[n] for n in _E))
    bad = undefined(grad)
    return {k: np.where(bad, F32(np.nan), out[k]).astype(F32) for k in PRINCIPAL_NAMES}


def polar_from_gradient_ref(grad):
    """(fields, folded): dict name -> float32 array of all seven outputs (NaN where the voxel is undefined or folded) and the mask
    of the defined voxels that are folded"""
    G = rows(grad)
    with np.errstate(all="ignore"):
        out, folded = polar_of_gradient(G)
    bad = undefined(grad)
    folded = folded & ~bad
    good = ~bad & ~folded
    return {k: np.where(good, out[k], F32(np.nan)).astype(F32) for k in POLAR_NAMES}, folded


def _fold_max(x):
    return float(np.fmax.reduce(x.ravel(), initial=F32(-np.inf)))


def _fold_min(x):
    return float(np.fmin.reduce(x.ravel(), initial=F32(np.inf)))


def principal_stats(fields):
    """the statistics of f3d_principal_from_gradient from principal_from_gradient_ref's result"""
    e1, e3, gmax = fields["e1"], fields["e3"], fields["gmax"]
    ok = ~np.isnan(e1)
    if not (np.isnan(e3[ok]).any() or np.isnan(gmax[ok]).any()):
        return principal_stats_ref(e1, e3, gmax)
    return {"defined": int(ok.sum()), "e1_max": _fold_max(e1[ok]), "e3_min": _fold_min(e3[ok]), "shear_max": _fold_max(gmax[ok])}


def polar_stats(fields, folded):
    """the statistics of f3d_polar_from_gradient from polar_from_gradient_ref's result"""
    theta, l1, l3 = fields["theta"], fields["l1"], fields["l3"]
    ok = ~np.isnan(l1)
    if not (np.isnan(theta[ok]).any() or np.isnan(l3[ok]).any()):
        return polar_stats_ref(fields, folded)
    return {"defined": int(ok.sum()), "folded": int(folded.sum()), "theta_max": _fold_max(theta[ok]), "l1_max": _fold_max(l1[ok]),
            "l3_min": _fold_min(l3[ok]), "theta_sum": float("nan")}
