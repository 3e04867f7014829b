"""Float32 numpy restatement of the principal strains of a displacement (include/f3d.h, f3d_principal_strain), the checker of the
kernel.

E comes from strain_ref (gradient_ref, fields_of_gradient): the very tensor f3d_flow_strain stores.  Rules 2-5 of the header follow,
vectorised over the voxels with np.where: five cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2), a rotation being skipped
where its off-diagonal is 0; three compare-exchanges; the sign rule; the statistics.  Every operation is one float32 numpy operation,
rounded on its own like the kernel's, so the two agree bit for bit (NaN positions, not payloads)."""
import numpy as np

from strain_ref import fields_of_gradient, gradient_ref

F32 = np.float32
NAMES = ("e1", "e2", "e3", "gmax", "d1x", "d1y", "d1z", "d3x", "d3y", "d3z")
GROUP = {"e1": "val", "e2": "val", "e3": "val", "gmax": "shear", "d1x": "dir1", "d1y": "dir1", "d1z": "dir1", "d3x": "dir3",
         "d3y": "dir3", "d3z": "dir3"}
SWEEPS = 5
_ONE, _TWO, _HALF, _ZERO = F32(1), F32(2), F32(0.5), F32(0)


def _rotate(A, V, p, q):
    """rule 2 for the pair (p, q): A a dict (i, j) i <= j -> array, V a 3 x 3 list of arrays [k][column]; in place"""
    r = 3 - p - q
    rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
    apq, app, aqq = A[(p, q)], A[(p, p)], A[(q, q)]
    skip = apq == _ZERO
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (_TWO * apq)
        t = _ONE / (np.abs(theta) + np.sqrt(theta * theta + _ONE))
        t = np.where(theta < _ZERO, -t, t)
        c = _ONE / np.sqrt(t * t + _ONE)
        s = t * c
        h = t * apq
        A[(p, p)] = np.where(skip, app, app - h)
        A[(q, q)] = np.where(skip, aqq, aqq + h)
        A[(p, q)] = np.where(skip, apq, _ZERO)
        arp, arq = A[rp], A[rq]
        A[rp] = np.where(skip, arp, c * arp - s * arq)
        A[rq] = np.where(skip, arq, s * arp + c * arq)
        for k in range(3):
            vp, vq = V[k][p], V[k][q]
            V[k][p] = np.where(skip, vp, c * vp - s * vq)
            V[k][q] = np.where(skip, vq, s * vp + c * vq)


def jacobi(e, sweeps=SWEEPS):
    """(A, V) after `sweeps` sweeps from E = (exx, eyy, ezz, exy, exz, eyz): A dict (i, j) -> array, V[k][column]"""
    e = [np.asarray(a, dtype=F32) for a in e]
    A = {(0, 0): e[0], (1, 1): e[1], (2, 2): e[2], (0, 1): e[3], (0, 2): e[4], (1, 2): e[5]}
    V = [[np.full_like(e[0], 1 if k == i else 0) for i in range(3)] for k in range(3)]
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            _rotate(A, V, p, q)
    return A, V


def _fix_sign(d):
    """rule 4 on a direction d = [x, y, z]"""
    with np.errstate(invalid="ignore"):
        lead = d[0]
        lead = np.where(np.abs(d[1]) > np.abs(lead), d[1], lead)
        lead = np.where(np.abs(d[2]) > np.abs(lead), d[2], lead)
        neg = lead < _ZERO
    return [np.where(neg, -x, x) for x in d]


def principal_of_tensor(e, sweeps=SWEEPS):
    """the ten outputs (dict name -> float32 array) of E = (exx, eyy, ezz, exy, exz, eyz): rules 2-4"""
    A, V = jacobi(e, sweeps)
    lam = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    col = [[V[k][i] for k in range(3)] for i in range(3)]       # col[i] = direction i = [x, y, z]
    with np.errstate(invalid="ignore"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            swap = lam[i] < lam[j]
            lam[i], lam[j] = np.where(swap, lam[j], lam[i]), np.where(swap, lam[i], lam[j])
            col[i], col[j] = ([np.where(swap, b, a) for a, b in zip(col[i], col[j])],
                              [np.where(swap, a, b) for a, b in zip(col[i], col[j])])
        gmax = _HALF * (lam[0] - lam[2])
    d1, d3 = _fix_sign(col[0]), _fix_sign(col[2])
    out = dict(zip(NAMES, (lam[0], lam[1], lam[2], gmax, *d1, *d3)))
    return {k: np.asarray(x, dtype=F32) for k, x in out.items()}


def tensor_ref(u, v, w):
    """((exx, eyy, ezz, exy, exz, eyz), defined) of a displacement, as f3d_flow_strain forms them"""
    G, defined = gradient_ref(u, v, w)
    f = fields_of_gradient(G)
    return tuple(f[n] for n in ("exx", "eyy", "ezz", "exy", "exz", "eyz")), defined


def principal_ref(u, v, w, sweeps=SWEEPS):
    """dict name -> float32 [z, y, x] array of all ten outputs (NaN where the voxel is undefined)"""
    e, defined = tensor_ref(u, v, w)
    out = principal_of_tensor(e, sweeps)
    return {k: np.where(defined, x, F32(np.nan)).astype(F32) for k, x in out.items()}


def principal_stats_ref(e1, e3, gmax):
    """the statistics of f3d_principal_strain (rule 5) from the restatement's e1, e3 and gmax"""
    ok = ~np.isnan(e1)
    n = int(ok.sum())
    nan = float("nan")
    return {
        "defined": n,
        "e1_max": float(e1[ok].max()) if n else nan,
        "e3_min": float(e3[ok].min()) if n else nan,
        "shear_max": float(gmax[ok].max()) if n else nan,
    }
