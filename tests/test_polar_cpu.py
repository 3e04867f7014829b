"""Local rotation and principal stretches without a GPU: the float32 restatement (tests/polar_ref.py, the checker of
f3d_polar_decomposition) on exact closed forms by bits, against float64 (numpy.linalg.svd polar factors, arccos of the trace,
arctan2), on frame indifference, on its consistency with the principal strains and on the missing-sample rules; the host library's
weak link to the device entry; the argument errors of flow3d --rotation; the symbols of both headers.

The float64 bounds are 4 x the worst value the restatement shows on this file's own seeded inputs; the measured worst values stand
beside them (MEASURED).  They bound the definition (float32 Jacobi, float32 products, the ATAN2 of the header); the kernel gets no
tolerance at all (tests/test_gpu_polar.py compares it with the restatement bit for bit)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import exact_ref as X
from polar_ref import HALFPI_F, NAMES, PI_F, atan2_ref, polar_of_gradient, polar_ref, polar_stats_ref, theta_sum_ref
from principal_ref import principal_of_tensor, principal_ref
from strain_ref import gradient_ref, same_bits, strain_ref
from test_strain_cpu import affine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

# worst values of the restatement on the inputs of this file (the largest over FAMILIES), measured on the CPU; each bound is 4 x its value
MEASURED = {
    "R": 9.88e-7,                 # max |R - R64| over the nine entries, R64 = W V^T of float64 svd(I + G) = W S V^T
    "angle": 4.93e-7,             # |theta - theta64| in radians, theta64 = arctan2(|skew part|, (trace - 1) / 2) of R64
    "vector": 1.76e-6,            # max |r - theta64 n64| over the three components
    "stretch": 3.19e-7,           # max |l_i - S_i|, S the singular values (descending)
    "orthogonal": 1.98e-6,        # max |R R^T - I| over the nine entries
    "atan2_eps": 2.85,            # |ATAN2(s, c) - arctan2(s, c)| / arctan2(s, c) in units of eps32
}
BOUND = {k: 4 * v for k, v in MEASURED.items()}


def random_rotations(rng, n, max_angle):
    """(Q [n, 3, 3], angle [n], axis [n, 3]) by Rodrigues' formula in float64"""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0, max_angle, size=n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0],
                                                                              -axis[:, 1], axis[:, 0])
    Q = np.eye(3) + np.sin(angle)[:, None, None] * K + (1 - np.cos(angle))[:, None, None] * (K @ K)
    return Q, angle, axis


def family(name):
    """the seeded inputs: name -> float32 gradients [n, 3, 3]"""
    if name.startswith("sine"):
        amp = float(name.split("-")[1])
        G, defined = gradient_ref(*X.smooth_displacement((40, 36, 33), "sine", amp=amp, seed=3))
        assert defined.all()
        return np.stack([np.stack([G[r][c].ravel() for c in range(3)], -1) for r in range(3)], -2).astype(F32)
    seeds = {"grad-0.3": 31, "grad-1e-3": 32, "grad-0.3-rot0.8": 33, "grad-0.3-rot2.5": 34, "grad-1e-3-rot0.8": 35, "grad-1e-3-rot2.5": 36}
    rng = np.random.default_rng(seeds[name])
    n = 100000
    amp = float(name.split("-rot")[0][len("grad-"):])
    G = rng.uniform(-amp, amp, size=(n, 3, 3))
    if "-rot" in name:
        Q, _, _ = random_rotations(rng, n, float(name.split("-rot")[1]))
        G = Q @ (np.eye(3) + G) - np.eye(3)
    return G.astype(F32)


FAMILIES = ["grad-0.3", "grad-1e-3", "grad-0.3-rot0.8", "grad-0.3-rot2.5", "grad-1e-3-rot0.8", "grad-1e-3-rot2.5", "sine-0.05", "sine-0.2"]


def as_lists(G):
    return [[G[:, r, c] for c in range(3)] for r in range(3)]


def polar64(G):
    """(R, theta, vector, stretches descending) of I + G in float64 from the singular value decomposition; the angle from arctan2 of
    the skew part and the trace, cross-checked against arccos of the trace"""
    F = np.eye(3) + G.astype(np.float64)
    assert (np.linalg.det(F) > 0).all()
    W, S, Vt = np.linalg.svd(F)
    R = W @ Vt
    c = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1)
    a = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    s = np.linalg.norm(a, axis=1)
    theta = np.arctan2(s, c)
    assert np.abs(np.arccos(np.clip(c, -1, 1)) - theta).max() < 1e-7          # arccos loses half the digits near 0 and pi
    vec = np.where(s[:, None] > 0, theta[:, None] / np.where(s > 0, s, 1)[:, None] * a, 0.0)
    return R, theta, vec, S


def measure(G):
    """the worst figures of the restatement on the float32 gradients G [n, 3, 3] against float64"""
    out, folded = polar_of_gradient(as_lists(G), with_parts=True)
    assert not folded.any()
    R64, theta64, vec64, S = polar64(G)
    R = np.stack([np.stack([np.asarray(out["R"][r][c], np.float64) for c in range(3)], -1) for r in range(3)], -2)
    l = np.stack([out["l1"], out["l2"], out["l3"]], -1).astype(np.float64)
    r = np.stack([out["rx"], out["ry"], out["rz"]], -1).astype(np.float64)
    assert (l[:, 0] >= l[:, 1]).all() and (l[:, 1] >= l[:, 2]).all()
    return {
        "R": float(np.abs(R - R64).max()),
        "angle": float(np.abs(out["theta"].astype(np.float64) - theta64).max()),
        "vector": float(np.abs(r - vec64).max()),
        "stretch": float(np.abs(l - S).max()),
        "orthogonal": float(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max()),
    }


@pytest.mark.parametrize("name", FAMILIES)
def test_against_float64_polar_factors(name):
    m = measure(family(name))
    print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in m.items()))
    for k, v in m.items():
        assert v <= BOUND[k], (k, m)


def atan2_pairs():
    """10^6 seeded (s, c) with s >= 0: the whole half plane at four scales, near both axes, and s down to 1e-8 beside c = 1"""
    rng = np.random.default_rng(41)
    n = 200000
    phi = rng.uniform(0, np.pi, size=n)
    rad = 10.0 ** rng.uniform(-3, 3, size=n)
    parts = [(rad * np.sin(phi), rad * np.cos(phi))]
    parts.append((np.sin(phi), np.cos(phi)))
    small = 10.0 ** rng.uniform(-8, -1, size=n)
    parts.append((small, np.ones(n)))                                  # angles down to 1e-8
    parts.append((small, -np.ones(n)))                                 # just below pi
    parts.append((np.ones(n), small * np.where(rng.random(n) < 0.5, -1, 1)))   # about pi / 2
    s = np.concatenate([p[0] for p in parts]).astype(F32)
    c = np.concatenate([p[1] for p in parts]).astype(F32)
    s[:4], c[:4] = (0, 0, 1, 1), (1, -1, 0, 1)                          # 0, pi and pi / 2 themselves, and pi / 4
    return s, c


def test_atan2_against_float64():
    s, c = atan2_pairs()
    assert s.size == 10 ** 6 and (s >= 0).all()
    got = atan2_ref(s, c)
    want = np.arctan2(s.astype(np.float64), c.astype(np.float64))
    assert got[0] == 0 and not np.signbit(got[0]) and got[1] == PI_F and got[2] == HALFPI_F
    ok = want > 0
    err = float((np.abs(got.astype(np.float64) - want)[ok] / want[ok]).max() / EPS32)
    print(f"ATAN2: worst relative error {err:.3g} eps32 on {s.size} pairs")
    assert err <= BOUND["atan2_eps"], err
    assert (got[~ok] == 0).all()
    assert (got >= 0).all() and (got <= PI_F).all()
    assert atan2_ref(F32(0), F32(0)) == PI_F                            # both zero: x = 0, c is not positive (no rotation has it)


# ---- exact closed forms, by bits ------------------------------------------------------------------------------------------------

def all_equal_bits(a, value):
    return same_bits(a, np.full(a.shape, value, F32))


def test_no_displacement_is_no_rotation_and_unit_stretch():
    zero = np.zeros((5, 6, 7), F32)
    got, folded = polar_ref(zero, zero, zero)
    assert not folded.any()
    for n in ("theta", "rx", "ry", "rz"):
        assert all_equal_bits(got[n], 0.0), n                          # +0: same_bits compares the sign bit too
    for n in ("l1", "l2", "l3"):
        assert all_equal_bits(got[n], 1.0), n
    st = polar_stats_ref(got, folded)
    assert st == {"defined": 5 * 6 * 7, "folded": 0, "theta_max": 0.0, "l1_max": 1.0, "l3_min": 1.0, "theta_sum": 0.0}


def test_an_axis_aligned_stretch_has_exact_stretches_and_no_rotation():
    """u = 0.25 x, v = -0.125 y: 1 + 2 E = diag(1.5625, 0.765625, 1), whose roots 1.25, 0.875 and 1 are float32 values"""
    shape = (9, 10, 11)
    got, folded = polar_ref(*affine([[0.25, 0, 0], [0, -0.125, 0], [0, 0, 0]], [0, 0, 0], shape))
    assert not folded.any()
    for n, want in (("theta", 0.0), ("rx", 0.0), ("ry", 0.0), ("rz", 0.0), ("l1", 1.25), ("l2", 1.0), ("l3", 0.875)):
        assert all_equal_bits(got[n], want), n
    st = polar_stats_ref(got, folded)
    assert st == {"defined": 9 * 10 * 11, "folded": 0, "theta_max": 0.0, "l1_max": 1.25, "l3_min": 0.875, "theta_sum": 0.0}


def test_a_quarter_turn_about_z_is_exact():
    """F = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]: E = 0, so U = I and R = F; the trace gives c = 0 and the skew part s = 1"""
    shape = (6, 7, 8)
    got, folded = polar_ref(*affine([[-1, -1, 0], [1, -1, 0], [0, 0, 0]], [3, -2, 0], shape))
    assert not folded.any()
    assert HALFPI_F == F32(np.pi / 2)
    for n, want in (("theta", HALFPI_F), ("rx", 0.0), ("ry", 0.0), ("rz", HALFPI_F), ("l1", 1.0), ("l2", 1.0), ("l3", 1.0)):
        assert all_equal_bits(got[n], want), n
    e = strain_ref(*affine([[-1, -1, 0], [1, -1, 0], [0, 0, 0]], [3, -2, 0], shape))
    assert not any(e[n].any() for n in ("vol", "exx", "eyy", "ezz", "exy", "exz", "eyz"))


def test_a_reflection_is_folded():
    shape = (4, 5, 6)
    got, folded = polar_ref(*affine([[-2, 0, 0], [0, 0, 0], [0, 0, 0]], [0, 0, 0], shape))
    assert folded.all()
    for n in NAMES:
        assert np.isnan(got[n]).all(), n
    st = polar_stats_ref(got, folded)
    assert st["defined"] == 0 and st["folded"] == 4 * 5 * 6 and st["theta_sum"] == 0.0
    assert all(np.isnan(st[k]) for k in ("theta_max", "l1_max", "l3_min"))
    # a collapse onto a plane: vol = -1 exactly, and m_0 = 0 is not positive either
    got, folded = polar_ref(*affine([[-1, 0, 0], [0, 0, 0], [0, 0, 0]], [0, 0, 0], shape))
    assert folded.all() and np.isnan(got["l1"]).all()


# ---- frame indifference ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_angle", [0.8, 2.5])
def test_a_rotated_stretch_gives_back_the_rotation_and_the_stretch(max_angle):
    """F = Q U0 with U0 symmetric positive definite: the decomposition is unique, so R = Q and the stretches are U0's"""
    rng = np.random.default_rng(int(max_angle * 10))
    n = 50000
    P, _, _ = random_rotations(rng, n, np.pi)
    lam0 = np.sort(rng.uniform(0.7, 1.4, size=(n, 3)), axis=1)[:, ::-1]
    U0 = P @ (lam0[:, :, None] * np.swapaxes(P, 1, 2))
    Q, angle, axis = random_rotations(rng, n, max_angle)
    G = (Q @ U0 - np.eye(3)).astype(F32)
    out, folded = polar_of_gradient(as_lists(G))
    assert not folded.any()
    l = np.stack([out["l1"], out["l2"], out["l3"]], -1).astype(np.float64)
    r = np.stack([out["rx"], out["ry"], out["rz"]], -1).astype(np.float64)
    worst = (np.abs(out["theta"] - angle).max(), np.abs(r - angle[:, None] * axis).max(), np.abs(l - lam0).max())
    print(f"up to {max_angle} rad: angle {worst[0]:.3g}, vector {worst[1]:.3g}, stretch {worst[2]:.3g}")
    assert worst[0] <= BOUND["angle"] and worst[1] <= BOUND["vector"] and worst[2] <= BOUND["stretch"], worst


# ---- consistency with the principal strains --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grad-0.3", "grad-0.3-rot2.5", "sine-0.2"])
def test_the_stretches_are_the_roots_of_the_principal_strains_by_bits(name):
    G = as_lists(family(name))
    out, folded = polar_of_gradient(G, with_parts=True)
    assert not folded.any()
    from principal_ref import jacobi
    A, _ = jacobi(out["e"])
    for i in range(3):                                                  # before ordering: l_i = sqrt(2 e_i + 1)
        assert same_bits(out["lam"][i], np.sqrt(F32(2) * A[(i, i)] + F32(1))), i
    p = principal_of_tensor(out["e"])
    for ln, en in (("l1", "e1"), ("l2", "e2"), ("l3", "e3")):           # the root is monotone, so ordering and root commute
        assert same_bits(out[ln], np.sqrt(F32(2) * p[en] + F32(1))), ln


def test_the_stretches_of_a_field_with_holes_and_folds():
    dims = (37, 21, 9)
    rng = np.random.default_rng(13)
    comps = [c * F32(8) for c in X.smooth_displacement(dims, "sine", amp=0.2, seed=5)]
    all_nan, one_nan = X.seam_holes(dims, rng, density=0.05)
    comps = X.with_holes(comps, all_nan, one_nan, which=2)
    got, folded = polar_ref(*comps)
    p = principal_ref(*comps)
    und = np.isnan(p["e1"])
    assert np.array_equal(und, X.predicted_undefined(all_nan | one_nan)) and und.any() and not und.all()
    assert folded.any() and not (folded & und).any()
    vol = strain_ref(*comps)["vol"]
    with np.errstate(invalid="ignore"):
        assert folded[vol <= -1].all()                                  # every voxel f3d_flow_strain counts as folded is folded here
    good = ~und & ~folded
    for n in NAMES:
        assert np.array_equal(np.isnan(got[n]), ~good), n
    with np.errstate(invalid="ignore"):
        for ln, en in (("l1", "e1"), ("l2", "e2"), ("l3", "e3")):
            assert same_bits(got[ln][good], np.sqrt(F32(2) * p[en][good] + F32(1))), ln
    st = polar_stats_ref(got, folded)
    assert st["defined"] == int(good.sum()) and st["folded"] == int(folded.sum())
    assert st["theta_max"] == float(np.nanmax(got["theta"])) and st["l3_min"] == float(np.nanmin(got["l3"]))
    exact = X.fsum(got["theta"][good].astype(np.float64))
    assert abs(st["theta_sum"] - exact) <= 1e-12 * exact                # the fixed order is a sum of the same numbers


def test_the_sum_follows_the_order_of_the_reduction():
    """one value per workgroup, then per fold thread: where every partial is a single number the fixed order is easy to write down"""
    theta = np.full((70, 9, 130), np.nan, F32)
    rng = np.random.default_rng(5)
    vals = rng.uniform(0, 3, size=(3, 3, 3)).astype(F32)
    theta[::32, ::4, ::64] = vals                                       # one voxel in each of the 3 x 3 x 3 workgroups
    part = np.zeros(256)                                                # 27 partials: threads 0 .. 26 hold one each, the tree adds
    part[:27] = vals.astype(np.float64).ravel()
    s = 128
    while s:
        part = part[:s] + part[s:2 * s]
        s //= 2
    want = float(part[0])
    assert theta_sum_ref(theta) == want
    assert theta_sum_ref(np.full((3, 3, 3), np.nan, F32)) == 0.0


@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 1, 9), (1, 1, 1), (2, 5, 1)])
def test_an_axis_of_size_one(shape):
    rng = np.random.default_rng(sum(shape))
    d = [rng.uniform(-0.2, 0.2, size=shape).astype(F32) for _ in range(3)]
    got, folded = polar_ref(*d)
    assert not folded.any() and not any(np.isnan(got[n]).any() for n in NAMES)
    if shape == (1, 1, 1):
        assert got["theta"][0, 0, 0] == 0 and got["l1"][0, 0, 0] == 1 and got["l3"][0, 0, 0] == 1


# ---- the weak link of the host library ---------------------------------------------------------------------------------------------

CASE = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["F3D_ROOT"])
    pkg = importlib.import_module("cuda-flow3d_amd")
    pkg._LIBDIR = os.environ["F3D_TEST_LIBDIR"]          # test-only: the host-memory stand-in
    W, H, D = 20, 18, 16
    f0, f1 = pkg.synth_pair(W, H, D)
    kw = dict(warp_levels_count=4, outer_iterations_count=2, inner_iterations_count=3)
    flow = pkg.OpticalFlow(); flow.initialize(W, H, D)
    flow.upload(f0, f1); flow.compute_resident(silent=True, **kw)
    u, v, w = flow.download()
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    for call in (lambda: flow.rotation("flow"), lambda: flow.rotation("flow", fields=("stretch",)),
                 lambda: pkg.polar_decomposition(u, v, w)):
        try:
            call(); raise SystemExit("a rotation call succeeded without f3d_polar_decomposition")
        except pkg.F3dError as e:
            assert "f3d_polar_decomposition" in str(e), str(e)
    # the C API itself, without the binding in between
    host = pkg.host()
    ptrs = (pkg._fp * 7)(*[np.empty((D, H, W), np.float32).ctypes.data_as(pkg._fp) for _ in range(7)])
    assert host.f3d_flow_polar_compute(flow._h, 0, 7, ptrs, None) != 0
    assert b"f3d_polar_decomposition" in host.f3d_host_last_error()
    try:
        flow.rotation("trajectory"); raise SystemExit("the rotation of a trajectory that was never started succeeded")
    except pkg.F3dError as e:
        assert "trajectory" in str(e), str(e)
    flow.rotation_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_polar_decomposition: libf3d_host.so built against it must still load (RTLD_NOW) and solve,
    and polar_decomposition, OpticalFlow.rotation and f3d_flow_polar_compute must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_polar_decomposition" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- flow3d --rotation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,needle", [(["--rotation", "angle,axis"], "usage"), (["--rotation", ""], "usage"),
                                          (["--rotation", "angle,,stretch"], "usage"), (["--rotation"], "usage"),
                                          (["--strain", "vol", "--rotation", "val"], "usage"),
                                          (["--rotation", "angle", "--partial"], "--rotation"),
                                          (["--rotation", "vector,stretch", "--concurrent", "2"], "--rotation")])
def test_flow3d_rotation_argument_errors(tmp_path, extra, needle):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-flow3d_amd"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for i in range(3):
        p = tmp_path / f"f{i}.raw"
        np.zeros((4, 4, 4), np.float32).tofile(p)
        paths.append(str(p))
    run = subprocess.run([EXE, "--dims", "4", "4", "4", "--f32", "--frames", *paths, "--out", str(tmp_path / "o")] + extra,
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 64, (run.returncode, run.stdout[-1000:], run.stderr[-1000:])
    assert needle in run.stdout and "usage" in run.stdout and "--rotation angle,vector,stretch" in run.stdout
    assert not any("rotation" in n or "strain" in n or "flow-" in n for n in os.listdir(tmp_path))


# ---- the headers -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_polar_decomposition"]),
                                              ("f3d_host.h", "host", ["f3d_flow_polar_compute", "f3d_flow_polar_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    assert not [n for n in have if not hasattr(handle, n)]


def test_the_binding_names_the_outputs_in_abi_order(f3d):
    assert f3d.POLAR_NAMES == NAMES
    assert f3d.POLAR_GROUPS == {"angle": 1, "vector": 2, "stretch": 4}
    assert f3d._polar_mask("angle,stretch") == 5 and f3d._polar_mask(("vector",)) == 2
    for bad in ("", "angle,", "val", ()):
        with pytest.raises(ValueError):
            f3d._polar_mask(bad)
    import ctypes as C
    assert C.sizeof(f3d.PolarStats) == 40
    assert callable(f3d.polar_decomposition) and callable(f3d.OpticalFlow.rotation) and callable(f3d.OpticalFlow.rotation_end)
    assert callable(f3d._polar_entry)
