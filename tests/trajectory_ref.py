"""Float32 numpy restatement of one trajectory step (include/f3d.h, f3d_compose_flow), the checker of the kernel.

For every voxel (x, y, z) of frame 0's grid, with acc the displacement so far and inc the next pair's flow (both [z, y, x]):
    p = (x + acc_u, y + acc_v, z + acc_w)                       one float32 add per axis
    p NaN or outside [0, W-1] x [0, H-1] x [0, D-1]  ->  acc = NaN in all three components
    else                                             ->  acc += trilinear sample of inc at p
The sample is k_warp's (registration_3d.cu:66-79): the same products and sums in the same order, every operation rounded to
float32 on its own, so this agrees with the kernel bit for bit (NaN positions, not payloads)."""
import numpy as np

F32 = np.float32


def compose_ref(acc, inc):
    """one step; returns the new (u, v, w) as float32 arrays (inputs untouched)"""
    au, av, aw = (np.array(a, dtype=F32) for a in acc)
    inc = [np.asarray(a, dtype=F32) for a in inc]
    d, h, w = au.shape
    z, y, x = np.meshgrid(np.arange(d, dtype=F32), np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    x_f, y_f, z_f = x + au, y + av, z + aw
    with np.errstate(invalid="ignore"):
        lost = (np.isnan(x_f) | np.isnan(y_f) | np.isnan(z_f) | (x_f < F32(0)) | (x_f > F32(w - 1)) | (y_f < F32(0)) |
                (y_f > F32(h - 1)) | (z_f < F32(0)) | (z_f > F32(d - 1)))
    keep = ~lost
    xf, yf, zf = x_f[keep], y_f[keep], z_f[keep]
    xi, yi, zi = (np.floor(t).astype(np.int64) for t in (xf, yf, zf))
    dx, dy, dz = xf - xi.astype(F32), yf - yi.astype(F32), zf - zi.astype(F32)
    x1, y1, z1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1), np.minimum(d - 1, zi + 1)
    one = F32(1)

    def sample(f):
        v0 = ((one - dx) * (one - dy) * f[zi, yi, xi] + (dx) * (one - dy) * f[zi, yi, x1] +
              (one - dx) * (dy) * f[zi, y1, xi] + (dx) * (dy) * f[zi, y1, x1])
        v1 = ((one - dx) * (one - dy) * f[z1, yi, xi] + (dx) * (one - dy) * f[z1, yi, x1] +
              (one - dx) * (dy) * f[z1, y1, xi] + (dx) * (dy) * f[z1, y1, x1])
        return (one - dz) * v0 + dz * v1

    out = []
    for a, f in zip((au, av, aw), inc):
        r = np.empty_like(a)
        r[lost] = np.nan
        r[keep] = a[keep] + sample(f)
        out.append(r)
    return tuple(out)


def compose_sequence_ref(flows):
    """the displacement after each of `flows` (a list of (u, v, w)), starting from zero"""
    acc = tuple(np.zeros_like(np.asarray(c, dtype=F32)) for c in flows[0])
    out = []
    for f in flows:
        acc = compose_ref(acc, f)
        out.append(acc)
    return out


def same_bits(a, b):
    """equal as float32 values with NaN at the same positions (payloads not compared)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
