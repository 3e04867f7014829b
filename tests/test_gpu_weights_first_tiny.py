"""The weights-first launch (k_wpair8<PAIR_PS>, f3d_solve_phi_ksi_sweep_fd) on phi numerators below 2^-100.

Its phi stage divides the nine numerators ((U[+1] - U[-1]) + dU[+1]) - dU[-1] by 2h through the reciprocal WITHOUT the guard that sends a wave
with a numerator 0 < |x| < 2^-100 down the IEEE road (each quotient is only squared: tests/test_udiv_square_cpu.py).  The one-stage launches
f3d_phi_ksi + f3d_solve_sweep keep the guard, the oracle divides as the reference does: phi, ksi and the three increments must equal both
bit for bit, over whole NaN-filled containers of pitch 256 (inputs outside the box are NaN, outputs outside it must keep their fill).

Inputs.  u, v, w are constant per plane in the left half of a plane and random in the right half, so the x and y numerators of the left half
are du[+1] - du[-1] alone (the z numerators are ordinary, except at the two z faces, where the mirror rule makes them exactly zero: there all
nine can be tiny at once).  du, dv, dw draw every voxel from five classes: +-0, subnormals of both signs, normals below 2^-100 of both signs,
values in [2^-100, 2^-98) (2^-100 itself among them), ordinary values.  The middle plane is ordinary throughout, with ONE voxel per row and
tile column whose x numerator of u is exactly a tiny value: a single lane of its wave.  The oracle's phi is finite everywhere (asserted).
"""
import numpy as np
import pytest

from conftest import bit_same

pytestmark = pytest.mark.gpu

H3 = (1.3, 0.9, 2.0)
ALPHA = 7.5
EPS = (0.001, 0.001)
FILL = 0xFFFFFFFF
TINY = np.float32(2.0 ** -100)

# (W, H, D), tile height, workgroups per round (0: the default)
CASES = [
    ((65, 14, 5), 4, 0),       # the halo column is the last column of the volume
    ((80, 30, 7), 12, 0),      # folded last tile column, 12-row tiles
    ((130, 26, 9), 8, 8),      # the folded tiles cut into z-chunks (rounds of eight workgroups)
    ((130, 26, 9), 12, 8),     # ... and the 12-row build on the same volume
]


def classed(rng, shape):
    """float32 values of the five classes, one draw per voxel"""
    n = int(np.prod(shape))
    kind = rng.choice(5, size=n, p=[0.25, 0.25, 0.25, 0.1, 0.15])
    sign = rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    bits = np.zeros(n, np.uint32)                                                                       # +-0
    sub = rng.integers(1, 1 << 23, n, dtype=np.uint32) >> rng.integers(0, 23, n, dtype=np.uint32)       # every subnormal binade
    bits = np.where(kind == 1, np.maximum(sub, 1), bits)
    bits = np.where(kind == 2, rng.integers(1 << 23, 27 << 23, n, dtype=np.uint32), bits)               # 2^-126 .. below 2^-100
    above = rng.integers(27 << 23, 29 << 23, n, dtype=np.uint32)
    above[::7] = 27 << 23                                                                               # 2^-100 itself
    bits = np.where(kind == 3, above, bits)
    out = (bits.astype(np.uint32) | sign).view(np.float32)
    out = np.where(kind == 4, rng.uniform(-0.5, 0.5, n).astype(np.float32), out)
    return out.reshape(shape)


def make_inputs(dims):
    """fx, fy, fz, ft are made on the device from f0, f1; returns the eight host containers (f0, f1, u, v, w, du, dv, dw) and the voxels
    (z, y, x) whose x numerator of u is the planted tiny value"""
    W, H, D = dims
    cdims = (256, H + 3, D + 1)
    rng = np.random.default_rng(W * 1000 + H * 10 + D)
    box = lambda lo, hi: rng.uniform(lo, hi, size=(D, H, W)).astype(np.float32)
    f0, f1 = box(0, 255), box(0, 255)
    flow = [box(-3, 3) for _ in range(3)]
    half = W // 2
    for a in flow:
        a[:, :, :half] = rng.uniform(-3, 3, size=(D, 1, 1)).astype(np.float32)
    inc = [classed(rng, (D, H, W)) for _ in range(3)]
    zs = D // 2
    for a in flow:
        a[zs] = rng.uniform(-3, 3, size=(H, W)).astype(np.float32)
    for a in inc:
        a[zs] = rng.uniform(-0.5, 0.5, size=(H, W)).astype(np.float32)
    planted = []
    tiny = classed(np.random.default_rng(7), (4096,))
    tiny = tiny[(np.abs(tiny) > 0) & (np.abs(tiny) < TINY)]
    for y in range(H):
        for x0 in range(0, W, 64):
            room = min(W, x0 + 64) - x0          # columns of this tile column
            if room < 3:
                continue
            x = x0 + 1 + (5 + 3 * y) % (room - 2)
            flow[0][zs, y, x + 1] = flow[0][zs, y, x - 1]
            inc[0][zs, y, x - 1] = 0
            inc[0][zs, y, x + 1] = tiny[(y * 5 + x0) % tiny.size]
            planted.append((zs, y, x))
    hosts = []
    for a in [f0, f1] + flow + inc:
        c = np.full((cdims[2], cdims[1], cdims[0]), np.nan, np.float32)
        c[:D, :H, :W] = a
        hosts.append(c)
    return cdims, hosts, planted


def numerators(hosts, dims):
    """the nine numerators with the reference's operations and its mirror rule, on the host (what the classes of the docstring mean)"""
    W, H, D = dims
    out = []
    for comp in range(3):
        U, dU = hosts[2 + comp][:D, :H, :W], hosts[5 + comp][:D, :H, :W]
        for axis, n in ((2, W), (1, H), (0, D)):
            ip = np.minimum(np.arange(n) + 1, n - 1)
            ip[n - 1] = n - 2
            im = np.abs(np.arange(n) - 1)
            p = lambda a, i: np.take(a, i, axis=axis)
            with np.errstate(under="ignore"):
                out.append(((p(U, ip) - p(U, im)) + p(dU, ip)) - p(dU, im))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """inputs and the oracle's phi, ksi and increments per volume: computed once, shared by the cases of a volume, never written"""
    made = {}
    for dims in sorted({c[0] for c in CASES}):
        cdims, hosts, planted = make_inputs(dims)
        W, H, D = dims
        e_phi, e_ksi = oracle.phi_ksi(*hosts, dims, H3, *EPS)
        e_inc = oracle.solve_sweep(*hosts, e_phi, e_ksi, dims, H3, ALPHA)
        assert np.isfinite(e_phi[:D, :H, :W]).all() and np.isfinite(e_ksi[:D, :H, :W]).all()
        assert all(np.isfinite(e[:D, :H, :W]).all() for e in e_inc)
        # the classes are there: zeros, tiny values of both signs (subnormal and normal), values just above 2^-100, and voxels whose
        # nine numerators are all tiny or zero; the planted voxels are the only tiny lanes of their rows
        nq = numerators(hosts, dims)
        mag = np.abs(np.stack(nq))
        assert (mag == 0).any() and ((mag > 0) & (mag < np.float32(2.0 ** -126))).any()
        assert ((mag >= np.float32(2.0 ** -126)) & (mag < TINY)).any() and ((mag >= TINY) & (mag < 4 * TINY)).any()
        assert (np.stack(nq)[(mag > 0) & (mag < TINY)] < 0).any() and (np.stack(nq)[(mag > 0) & (mag < TINY)] > 0).any()
        assert (mag < TINY).all(axis=0).any()
        tiny_lane = ((mag > 0) & (mag < TINY)).any(axis=0)
        for z, y, x in planted:
            lo = x // 64 * 64
            assert tiny_lane[z, y, x] and tiny_lane[z, y, lo:lo + 64].sum() == 1
        made[dims] = (cdims, hosts, [e_phi, e_ksi] + list(e_inc))
    return made


def outside_is_fill(g, dims):
    W, H, D = dims
    outside = np.ones(g.shape, bool)
    outside[:D, :H, :W] = False
    return bool((np.ascontiguousarray(g).view(np.uint32)[outside] == FILL).all())


@pytest.mark.parametrize("dims,ty,per_round", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tiny_numerators_bit_for_bit(f3d, cases, monkeypatch, dims, ty, per_round):
    monkeypatch.setenv("F3D_PAIR8_TY", str(ty))
    if per_round:
        monkeypatch.setenv("F3D_PAIR8_ROUND", str(per_round))
    else:
        monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    W, H, D = dims
    cdims, hosts, expect = cases[dims]
    hip = f3d.hip()
    cont = f3d.Containers(*cdims)
    cont.alloc(fill=0xFF)
    cont.set_current()
    try:
        ptr = []
        for a in hosts:
            p = cont.new()
            cont.upload(p, a)
            ptr.append(p)
        fd = [cont.new() for _ in range(4)]
        f3d.check(hip.f3d_frame_derivatives(ptr[0], ptr[1], *dims, *H3, *fd, None))
        outs = [cont.new() for _ in range(5)]      # phi, ksi, three increments
        f3d.check(f3d.solve_phi_ksi_sweep_fd_entry()(*fd, *ptr[2:], W, H, D, *H3, ALPHA, *EPS, *outs, None))
        one = [cont.new() for _ in range(5)]       # the one-stage launches: they keep the guard
        f3d.check(hip.f3d_phi_ksi(*ptr, W, H, D, *H3, *EPS, one[0], one[1], None))
        f3d.check(hip.f3d_solve_sweep(*ptr, one[0], one[1], W, H, D, *H3, ALPHA, *one[2:], None))
        f3d.sync()
        for name, p, q, e in zip(("phi", "ksi", "du", "dv", "dw"), outs, one, expect):
            g, o = cont.download(p, cdims), cont.download(q, cdims)
            bad_e = int((g[:D, :H, :W].view(np.uint32) != e[:D, :H, :W].view(np.uint32)).sum())
            bad_o = int((g[:D, :H, :W].view(np.uint32) != o[:D, :H, :W].view(np.uint32)).sum())
            print(f"{name}: {bad_e} voxels differ from the oracle, {bad_o} from the one-stage launches")
            assert bit_same(g[:D, :H, :W], e[:D, :H, :W]), f"{name}: differs from the oracle"
            assert bit_same(g[:D, :H, :W], o[:D, :H, :W]), f"{name}: differs from f3d_phi_ksi + f3d_solve_sweep"
            assert outside_is_fill(g, dims), f"{name}: written outside the box"
        for p, a in zip(ptr, hosts):
            assert bit_same(cont.download(p, cdims), a), "an input was written"
    finally:
        f3d.sync()
        cont.free()
