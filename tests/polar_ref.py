"""Float32 numpy restatement of the polar decomposition of a displacement's deformation gradient (include/f3d.h,
f3d_polar_decomposition), the checker of the kernel.

G and the undefined set come from strain_ref.gradient_ref, vol and E from strain_ref.fields_of_gradient (the very expressions of
f3d_flow_strain), (A, V) from principal_ref.jacobi (rule 2 of f3d_principal_strain).  Rules 3-6 of the header follow, vectorised over
the voxels with np.where.  Every operation is one float32 numpy operation, rounded on its own like the kernel's, and only + - * /
and sqrt occur, so the two agree bit for bit (NaN positions, not payloads).  The statistics restate the reduction's fixed order too,
so theta_sum agrees to the last bit."""
import numpy as np

from principal_ref import jacobi
from strain_ref import fields_of_gradient, gradient_ref

F32 = np.float32
NAMES = ("theta", "rx", "ry", "rz", "l1", "l2", "l3")
GROUP = {"theta": "angle", "rx": "vector", "ry": "vector", "rz": "vector", "l1": "stretch", "l2": "stretch", "l3": "stretch"}
_ZERO, _ONE, _TWO, _FOUR, _HALF = F32(0), F32(1), F32(2), F32(4), F32(0.5)
K3, K5, K7, K9 = (_ONE / F32(n) for n in (3, 5, 7, 9))
PI_F, HALFPI_F = F32(np.pi), F32(np.pi / 2)
assert [int(k.view(np.uint32)) for k in (K3, K5, K7, K9, PI_F, HALFPI_F)] == [0x3EAAAAAB, 0x3E4CCCCD, 0x3E124925, 0x3DE38E39,
                                                                              0x40490FDB, 0x3FC90FDB]
# the geometry of the reduction: a wave on 64 x, 4 rows per workgroup, 32 planes per run, 256 threads in the fold
BX, BY, BZ, FOLD = 64, 4, 32, 256


def atan2_ref(s, c):
    """rule 6: ATAN2(s, c) for s >= 0 (float32 arrays)"""
    s, c = np.asarray(s, dtype=F32), np.asarray(c, dtype=F32)
    with np.errstate(all="ignore"):
        big = np.abs(c) >= s
        x = np.where(big, s / c, c / s)
        x = np.where((s == _ZERO) & (c == _ZERO), _ZERO, x).astype(F32)
        for _ in range(2):
            x = x / (_ONE + np.sqrt(x * x + _ONE))
        z = x * x
        p = (((z * K9 - K7) * z + K5) * z - K3) * z + _ONE
        t = _FOUR * (x * p)
        return np.where(big, np.where(c > _ZERO, t, PI_F + t), HALFPI_F - t).astype(F32)


def polar_of_gradient(G, with_parts=False):
    """rules 1-6 on a gradient G[r][c] (float32 arrays of one shape): (out, folded) with out the seven outputs before any masking
    (dict name -> array) and folded the mask of rule 3.  with_parts: also "lam" (the three stretches before ordering), "R" (3 x 3
    list), "e" (the tensor's six components) and "vol"."""
    G = [[np.asarray(g, dtype=F32) for g in row] for row in G]
    f = fields_of_gradient(G)
    e = tuple(f[n] for n in ("exx", "eyy", "ezz", "exy", "exz", "eyz"))
    A, V = jacobi(e)
    with np.errstate(all="ignore"):
        m = [_TWO * A[(i, i)] + _ONE for i in range(3)]
        folded = f["vol"] <= F32(-1)
        for mi in m:
            folded = folded | ~(mi > _ZERO)
        lam = [np.sqrt(mi) for mi in m]
        l = list(lam)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            swap = l[i] < l[j]
            l[i], l[j] = np.where(swap, l[j], l[i]), np.where(swap, l[i], l[j])
        q = [_ONE / x for x in lam]
        ui = [[((V[r][0] * q[0]) * V[c][0] + (V[r][1] * q[1]) * V[c][1]) + (V[r][2] * q[2]) * V[c][2] for c in range(3)]
              for r in range(3)]
        fm = [[G[r][c] + _ONE if r == c else G[r][c] for c in range(3)] for r in range(3)]
        R = [[(fm[r][0] * ui[0][c] + fm[r][1] * ui[1][c]) + fm[r][2] * ui[2][c] for c in range(3)] for r in range(3)]
        cs = _HALF * (((R[0][0] + R[1][1]) + R[2][2]) - _ONE)
        a = [_HALF * (R[2][1] - R[1][2]), _HALF * (R[0][2] - R[2][0]), _HALF * (R[1][0] - R[0][1])]
        sn = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        theta = atan2_ref(sn, cs)
        k = theta / sn
        r = [np.where(sn == _ZERO, _ZERO, k * ak) for ak in a]
    out = dict(zip(NAMES, (theta, *r, *l)))
    out = {n: np.asarray(x, dtype=F32) for n, x in out.items()}
    if with_parts:
        out.update(lam=lam, R=R, e=e, vol=f["vol"])
    return out, folded


def polar_ref(u, v, w):
    """(fields, folded): dict name -> float32 [z, y, x] array of all seven outputs (NaN where the voxel is undefined or folded) and
    the mask of the defined voxels that are folded"""
    G, defined = gradient_ref(u, v, w)
    out, folded = polar_of_gradient(G)
    folded = folded & defined
    good = defined & ~folded
    return {k: np.where(good, x, F32(np.nan)).astype(F32) for k, x in out.items()}, folded


def theta_sum_ref(theta):
    """the double sum of the defined theta in the reduction's order: per lane along its run of planes, the wave's butterfly, the
    workgroup's waves in sequence, then the fold (thread t takes t, t + 256, ...; the halving tree)"""
    d, h, w = theta.shape
    gz, gy, gx = -(-d // BZ), -(-h // BY), -(-w // BX)
    t = np.zeros((gz * BZ, gy * BY, gx * BX), np.float64)            # theta >= +0: adding +0 for an absent voxel changes nothing
    t[:d, :h, :w] = np.where(np.isnan(theta), 0.0, theta.astype(np.float64))
    t = t.reshape(gz, BZ, gy, BY, gx, BX)
    lane = np.zeros((gz, gy, BY, gx, BX), np.float64)
    for z in range(BZ):
        lane = lane + t[:, z]
    o = BX // 2
    while o:                                                         # lane 0 of x + shfl_xor(x, o), o = 32 .. 1
        lane = lane[..., :o] + lane[..., o:2 * o]
        o //= 2
    wave = lane[..., 0]                                              # [gz, gy, BY, gx]
    block = wave[:, :, 0]
    for i in range(1, BY):
        block = block + wave[:, :, i]
    part = block.reshape(-1)                                         # (bz * gy + by) * gx + bx
    n = part.size
    pad = np.zeros(-(-n // FOLD) * FOLD, np.float64)
    pad[:n] = part
    acc = np.zeros(FOLD, np.float64)
    for row in pad.reshape(-1, FOLD):
        acc = acc + row
    s = FOLD // 2
    while s:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def polar_stats_ref(fields, folded):
    """the statistics of f3d_polar_decomposition from polar_ref's result"""
    theta, l1, l3 = fields["theta"], fields["l1"], fields["l3"]
    ok = ~np.isnan(l1)
    n = int(ok.sum())
    nan = float("nan")
    return {
        "defined": n,
        "folded": int(folded.sum()),
        "theta_max": float(theta[ok].max()) if n else nan,
        "l1_max": float(l1[ok].max()) if n else nan,
        "l3_min": float(l3[ok].min()) if n else nan,
        "theta_sum": theta_sum_ref(theta) if n else 0.0,
    }
