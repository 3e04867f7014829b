"""Restatements for the solves that start from a given displacement.

 * pyramid(): OpticalFlowE::ComputeFlow assembled in Python from the oracle's operators (gaussian, resample, warp, phi_ksi,
   solve_sweep, add, median), with an optional initial flow.  Without one it is oracle.compute_flow bit for bit; with one the first
   level's flow is the initial flow, copied when that level is level 0 and resampled from the original size otherwise (also when
   the level's box has the original's dimensions).  Values are never rescaled.
 * initial_flow(): f3d_initial_flow of include/f3d.h in numpy, float32 throughout.
 * test_pair(): three blobs and a ripple shifted by (6, -4, 3), and the constant guess (5, -3, 2).
"""
import numpy as np

from oracle import oracle as orc


def pyramid(frame0, frame1, initial=None, **kw):
    """(u, v, w) on dense [D, H, W] float32 volumes; initial: None or three such volumes"""
    p = dict(orc.DEFAULT_PARAMS)
    p.update(kw)
    f0 = np.ascontiguousarray(frame0, np.float32)
    f1 = np.ascontiguousarray(frame1, np.float32)
    D, H, W = f0.shape
    whole = (W, H, D)
    if p["gaussian_sigma"] > 0.0:
        f0 = orc.gaussian(f0, whole, p["gaussian_sigma"])
        f1 = orc.gaussian(f1, whole, p["gaussian_sigma"])
    levels = min(int(p["warp_levels_count"]), orc.max_warp_level(W, H, D, p["warp_scale_factor"]))
    if initial is None:
        flow = [np.zeros_like(f0) for _ in range(3)]
    else:
        flow = [np.ascontiguousarray(a, np.float32).copy() for a in initial]
    prev = None
    first = True
    for level in range(levels - 1, -1, -1):
        cur, h = orc.level_geometry(W, H, D, p["warp_scale_factor"], level)
        if level == 0:
            l0, l1 = f0, f1
        else:
            l0, l1 = orc.resample(f0, whole, cur), orc.resample(f1, whole, cur)
        if first:
            if initial is not None and level != 0:
                flow = [orc.resample(a, whole, cur) for a in flow]
        else:
            flow = [orc.resample(a, prev, cur) for a in flow]
        first = False
        l1 = orc.warp(l0, l1, *flow, cur, h)
        du, dv, dw = (np.zeros_like(f0) for _ in range(3))
        for _ in range(int(p["outer_iterations_count"])):
            phi, ksi = orc.phi_ksi(l0, l1, *flow, du, dv, dw, cur, h, p["equation_smoothness"], p["equation_data"])
            for _ in range(int(p["inner_iterations_count"])):
                du, dv, dw = orc.solve_sweep(l0, l1, *flow, du, dv, dw, phi, ksi, cur, h, p["equation_alpha"])
        for a, b in zip(flow, (du, dv, dw)):
            orc.add(a, b, cur)
        r = int(p["median_radius"])
        if r != 1:
            rr = r - 1 if r % 2 == 0 else r
            assert 3 <= rr <= 7, "the restatement covers the radii the median operator filters with"
            flow = [orc.median(a, cur, rr) for a in flow]
        prev = cur
    return tuple(flow)


def box_of(a, dims):
    w, h, d = dims
    return a[:d, :h, :w]


def initial_flow(u, v, w):
    """((out_u, out_v, out_w), dict(voxels, replaced, leaving, max_abs)) of dense [D, H, W] float32 volumes"""
    u, v, w = (np.ascontiguousarray(a, np.float32) for a in (u, v, w))
    D, H, W = u.shape
    finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(w)
    out = tuple(np.where(finite, a, np.float32(0.0)).astype(np.float32) for a in (u, v, w))
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        px, py, pz = (x + u).astype(np.float32), (y + v).astype(np.float32), (z + w).astype(np.float32)
        outside = (px < 0) | (px > np.float32(W - 1)) | (py < 0) | (py > np.float32(H - 1)) | (pz < 0) | (pz > np.float32(D - 1))
    largest = np.float32(0.0)
    if finite.any():
        largest = max(np.float32(np.abs(a[finite]).max()) for a in (u, v, w))
    info = dict(voxels=int(u.size), replaced=int((~finite).sum()), leaving=int((finite & outside).sum()), max_abs=np.float32(largest))
    return out, info


def initial_flow_by_loop(u, v, w):
    """the same, voxel by voxel with Python scalars of float32: the check of the vectorised restatement"""
    D, H, W = u.shape
    out = tuple(np.empty_like(a) for a in (u, v, w))
    replaced = leaving = 0
    largest = np.float32(0.0)
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    c = (u[z, y, x], v[z, y, x], w[z, y, x])
                    if all(np.isfinite(a) for a in c):
                        p = (f32(x) + c[0], f32(y) + c[1], f32(z) + c[2])
                        if any(q < 0 or q > f32(n - 1) for q, n in zip(p, (W, H, D))):
                            leaving += 1
                        largest = max([largest] + [abs(a) for a in c])
                    else:
                        c = (f32(0.0),) * 3
                        replaced += 1
                    for o, a in zip(out, c):
                        o[z, y, x] = a
    return out, dict(voxels=D * H * W, replaced=replaced, leaving=leaving, max_abs=f32(largest))


PAIR_SHAPE = (24, 40, 48)      # [z, y, x]
PAIR_SHIFT = (6.0, -4.0, 3.0)  # x, y, z
PAIR_GUESS = (5.0, -3.0, 2.0)


def _image(shape, shift):
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y, z = x - shift[0], y - shift[1], z - shift[2]

    def blob(c, sigma):
        return np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2.0 * sigma ** 2))

    img = (180.0 * blob((0.4 * w, 0.5 * h, 0.5 * d), w / 7.0) + 90.0 * blob((0.7 * w, 0.3 * h, 0.4 * d), w / 10.0) +
           70.0 * blob((0.3 * w, 0.75 * h, 0.6 * d), w / 9.0) + 25.0 * np.sin(0.45 * x) * np.cos(0.4 * y) * np.cos(0.5 * z))
    return img.astype(np.float32)


def test_pair(shape=PAIR_SHAPE, shift=PAIR_SHIFT):
    """(f0, f1) with f1(x) = f0(x - shift): the flow of the pair is `shift` everywhere"""
    return _image(shape, (0.0, 0.0, 0.0)), _image(shape, shift)


test_pair.__test__ = False  # a fixture's maker, not a test


def constant_flow(shape, value):
    return tuple(np.full(shape, c, np.float32) for c in value)


def rms_error(flow, truth=PAIR_SHIFT):
    """rms of the vector error against a constant displacement over [6:-6, 8:-8, 8:-8]"""
    e = sum((a[6:-6, 8:-8, 8:-8].astype(np.float64) - t) ** 2 for a, t in zip(flow, truth))
    return float(np.sqrt(e.mean()))
