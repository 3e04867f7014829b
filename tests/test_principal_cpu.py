"""Principal strains without a GPU: the float32 restatement (tests/principal_ref.py, the checker of f3d_principal_strain) against
exact closed forms, against float64 numpy.linalg.eigh of the same float32 tensor, on the missing-sample rules and its invariants;
the host library's weak link to the device entry; the argument errors of flow3d --principal; the symbols of both headers.

The float64 bounds are 4 x the worst value the restatement shows on this file's own seeded inputs; the measured worst values stand
beside them (MEASURED).  They bound the definition (five Jacobi sweeps in float32); the kernel gets no tolerance at all
(tests/test_gpu_principal.py compares it with the restatement bit for bit)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import exact_ref as X
from principal_ref import NAMES, jacobi, principal_of_tensor, principal_ref, principal_stats_ref, tensor_ref
from strain_ref import fields_of_gradient, strain_ref
from test_strain_cpu import affine, grid, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu_device")
EXE = os.path.join(ROOT, "cuda-flow3d_amd", "bin", "flow3d")
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

# worst values of the restatement on the inputs of this file (the largest over INPUTS), measured on the CPU; each bound is 4 x its value
MEASURED = {
    "eigenvalue": 3.57e-7,        # max_i |e_i - lambda_i| / max |lambda|, lambda = float64 eigvalsh of the float32 E
    "orthonormal": 9.53e-7,       # max(|d1.d1 - 1|, |d3.d3 - 1|, |d1.d3|)
    "residual": 3.89e-7,          # max(|E d1 - e1 d1|_inf, |E d3 - e3 d3|_inf) / max |lambda|
    "trace_ulps": 4.0,            # |((e1 + e2) + e3) - ((exx + eyy) + ezz)| in float32 ulps of max |lambda|
    "eq_ulps": 4.0,               # |eq of the principal values - eq of E| in float32 ulps of max |lambda|
}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
SEPARATION = 1e-3                 # a direction is compared where its eigenvalue is this far (x max |lambda|) from the other two


def tensors_of_gradients(G):
    """(exx .. eyz) of gradients G[n, 3, 3] (float32), through strain_ref's expressions"""
    f = fields_of_gradient([[G[:, r, c].astype(F32) for c in range(3)] for r in range(3)])
    return tuple(f[n] for n in ("exx", "eyy", "ezz", "exy", "exz", "eyz"))


def family(name):
    """the seeded inputs: name -> (exx .. eyz) as float32 arrays"""
    if name.startswith("sine"):
        amp = float(name.split("-")[1])
        e, defined = tensor_ref(*X.smooth_displacement((40, 36, 33), "sine", amp=amp, seed=3))
        assert defined.all()
        return e
    rng = np.random.default_rng({"small": 21, "large": 22, "isotropic": 23, "ulps": 23}[name])
    n = 100000
    if name == "small":          # gradients with entries up to 0.3, at four scales
        G = np.concatenate([rng.uniform(-0.3, 0.3, size=(n // 4, 3, 3)) * s for s in (1.0, 1e-1, 1e-2, 1e-3)])
        return tensors_of_gradients(G.astype(F32))
    if name == "large":          # gradients with entries up to 3
        return tensors_of_gradients(rng.uniform(-3, 3, size=(n, 3, 3)).astype(F32))
    # nearly isotropic: c I + a symmetric perturbation of 1e-6 ("isotropic"), or of 1e-6 |c|, a few float32 ulps of c ("ulps")
    c = rng.uniform(0.05, 0.3, size=n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p = rng.uniform(-1e-6, 1e-6, size=(6, n)) * (np.abs(c) if name == "ulps" else 1.0)
    return tuple((np.where(i < 3, c, 0.0) + p[i]).astype(F32) for i in range(6))


INPUTS = ["sine-0.05", "sine-0.2", "small", "large", "isotropic"]


def matrices(e):
    """float64 [n, 3, 3] symmetric matrices of the float32 components"""
    exx, eyy, ezz, exy, exz, eyz = (np.asarray(a, np.float64).ravel() for a in e)
    return np.stack([np.stack([exx, exy, exz], -1), np.stack([exy, eyy, eyz], -1), np.stack([exz, eyz, ezz], -1)], -2)


def measure(e):
    """the worst figures of the restatement on the tensors e against float64 eigh, and the share of voxels left out of the
    direction figures because e1 or e3 is not separated"""
    got = {k: np.asarray(v, np.float64).ravel() for k, v in principal_of_tensor(e).items()}
    M = matrices(e)
    lam = np.linalg.eigvalsh(M)[:, ::-1]                        # descending
    scale = np.abs(lam).max(axis=1)
    assert (scale > 0).all()
    val = np.stack([got["e1"], got["e2"], got["e3"]], -1)
    eig = (np.abs(val - lam).max(axis=1) / scale).max()
    sep = (np.minimum(lam[:, 0] - lam[:, 1], lam[:, 1] - lam[:, 2]) > SEPARATION * scale)
    d1 = np.stack([got["d1x"], got["d1y"], got["d1z"]], -1)[sep]
    d3 = np.stack([got["d3x"], got["d3y"], got["d3z"]], -1)[sep]
    out = {"eigenvalue": float(eig), "left_out": float(1 - sep.mean())}
    if sep.any():
        dot = lambda a, b: np.einsum("ni,ni->n", a, b)
        out["orthonormal"] = float(max(np.abs(dot(d1, d1) - 1).max(), np.abs(dot(d3, d3) - 1).max(), np.abs(dot(d1, d3)).max()))
        r1 = np.abs(np.einsum("nij,nj->ni", M[sep], d1) - val[sep, 0:1] * d1).max(axis=1)
        r3 = np.abs(np.einsum("nij,nj->ni", M[sep], d3) - val[sep, 2:3] * d3).max(axis=1)
        out["residual"] = float((np.maximum(r1, r3) / scale[sep]).max())
        # the directions themselves against eigh's, up to sign: |sin| of the angle is bounded by residual / separation
        _, vec = np.linalg.eigh(M[sep])
        for d, v in ((d1, vec[:, :, 2]), (d3, vec[:, :, 0])):
            sin = np.linalg.norm(np.cross(d, v), axis=1)
            assert sin.max() <= 2 * BOUND["residual"] / SEPARATION, sin.max()
    return out


@pytest.mark.parametrize("name", INPUTS)
def test_against_float64_eigh(name):
    m = measure(family(name))
    print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in m.items()))
    assert m["eigenvalue"] <= BOUND["eigenvalue"], m
    if name == "isotropic":                                   # deliberately degenerate: held to the eigenvalue bound only
        assert m["left_out"] > 0.9, m
        return
    assert m["left_out"] < 0.01, m
    assert m["orthonormal"] <= BOUND["orthonormal"], m
    assert m["residual"] <= BOUND["residual"], m


@pytest.mark.parametrize("name", INPUTS)
def test_five_sweeps_leave_no_off_diagonal(name):
    """what lets the kernel stop a wave early and the header fix the sweep count: after five sweeps every off-diagonal is exactly 0
    (and after three it is not, so the count is not slack)"""
    e = family(name)
    A, _ = jacobi(e)
    for pq in ((0, 1), (0, 2), (1, 2)):
        assert not np.asarray(A[pq]).any(), pq
    if name != "isotropic":
        A3, _ = jacobi(e, sweeps=3)
        assert any(np.asarray(A3[pq]).any() for pq in ((0, 1), (0, 2), (1, 2)))


def test_diagonals_equal_to_a_few_ulps_leave_next_to_nothing():
    """The one family found that five sweeps do not finish: diagonals that differ by a few float32 ulps with off-diagonals of the same
    size.  Where app == aqq after rounding a rotation turns by 45 degrees and only moves the other two off-diagonals around, so they
    shrink geometrically, not quadratically: 1 tensor in 100000 keeps an off-diagonal of 2e-33 max |lambda| (measured).  What is
    left must be below eps32^2 max |lambda|, where it cannot reach the last bit of an eigenvalue; the eigenvalue bound holds as well."""
    e = family("ulps")
    A, _ = jacobi(e)
    scale = np.maximum.reduce([np.abs(np.asarray(A[(i, i)], np.float64)) for i in range(3)])
    off = np.maximum.reduce([np.abs(np.asarray(A[pq], np.float64)) for pq in ((0, 1), (0, 2), (1, 2))])
    print(f"ulps: {float((off != 0).mean()):.3g} of the tensors keep an off-diagonal, the largest {float((off / scale).max()):.3g} max |lambda|")
    assert (off <= EPS32 ** 2 * scale).all()
    assert (off != 0).mean() < 1e-3
    assert measure(e)["eigenvalue"] <= BOUND["eigenvalue"]


def ulps_of_scale(diff, scale):
    return np.abs(diff.astype(np.float64)) / (np.spacing(scale.astype(F32)).astype(np.float64))


@pytest.mark.parametrize("name", INPUTS)
def test_invariants(name):
    """trace and equivalent strain do not depend on the frame: the principal values give back those of E"""
    e = [np.asarray(a, F32).ravel() for a in family(name)]
    got = {k: v.ravel() for k, v in principal_of_tensor(e).items()}
    scale = np.maximum(np.abs(got["e1"]), np.abs(got["e3"]))
    trace = ulps_of_scale(((got["e1"] + got["e2"]) + got["e3"]) - ((e[0] + e[1]) + e[2]), scale).max()

    def eq(a, b, c, off):
        m = ((a + b) + c) / F32(3)
        x, y, z = a - m, b - m, c - m
        return np.sqrt((((x * x + y * y) + z * z) + F32(2) * off) / F32(1.5))

    zero = np.zeros_like(e[0])
    eqd = ulps_of_scale(eq(got["e1"], got["e2"], got["e3"], zero) - eq(e[0], e[1], e[2], (e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]),
                        scale).max()
    print(f"{name}: trace {trace:.3g} ulps, eq {eqd:.3g} ulps")
    assert trace <= BOUND["trace_ulps"], trace
    assert eqd <= BOUND["eq_ulps"], eqd
    assert (got["e1"] >= got["e2"]).all() and (got["e2"] >= got["e3"]).all()
    assert np.array_equal(got["gmax"], F32(0.5) * (got["e1"] - got["e3"]))


# ---- exact closed forms -----------------------------------------------------------------------------------------------------------

def test_an_axis_aligned_stretch_is_exact_everywhere():
    """dyadic diagonal G: no off-diagonal, so no rotation happens and every figure is exact, faces included"""
    shape = (9, 10, 11)
    d = affine([[0.25, 0, 0], [0, 0, 0], [0, 0, -0.5]], [0, 0, 0], shape)
    got = principal_ref(*d)
    want = {"e1": 0.28125, "e2": 0.0, "e3": -0.375, "gmax": 0.328125, "d1x": 1, "d1y": 0, "d1z": 0, "d3x": 0, "d3y": 0, "d3z": 1}
    for n in NAMES:
        assert np.array_equal(got[n], np.full(shape, want[n], F32)), n
    st = principal_stats_ref(got["e1"], got["e3"], got["gmax"])
    assert st == {"defined": 9 * 10 * 11, "e1_max": 0.28125, "e3_min": -0.375, "shear_max": 0.328125}


def test_the_order_of_axis_aligned_stretches_and_of_equal_values():
    shape = (4, 4, 4)
    # smallest first on the grid's axes: the exchanges bring e1 to the front and its column with it
    got = principal_ref(*affine([[-0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.5]], [1, 2, 3], shape))
    assert (got["e1"] == F32(0.625)).all() and (got["e2"] == F32(0.28125)).all() and (got["e3"] == F32(-0.375)).all()
    assert (got["d1z"] == 1).all() and not got["d1x"].any() and not got["d1y"].any()
    assert (got["d3x"] == 1).all() and not got["d3y"].any() and not got["d3z"].any()
    # two equal values keep their axis order: e1 = e2 on x and y gives d1 = x; e2 = e3 on y and z gives d3 = z
    got = principal_ref(*affine([[0.25, 0, 0], [0, 0.25, 0], [0, 0, -0.5]], [0, 0, 0], shape))
    assert (got["e1"] == got["e2"]).all() and (got["d1x"] == 1).all() and (got["d3z"] == 1).all()
    got = principal_ref(*affine([[0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.25]], [0, 0, 0], shape))
    assert (got["e2"] == got["e3"]).all() and (got["d1x"] == 1).all() and (got["d3z"] == 1).all() and not got["d3y"].any()
    # no strain at all: three zeros, the grid's axes
    zero = np.zeros(shape, F32)
    got = principal_ref(zero, zero, zero)
    assert not any(got[n].any() for n in ("e1", "e2", "e3", "gmax")) and (got["d1x"] == 1).all() and (got["d3z"] == 1).all()


@pytest.mark.parametrize("s", [0.25, -0.125])
def test_a_stretch_along_an_oblique_direction(s):
    """G = s n n^T: E = (s + s^2 / 2) n n^T, so one principal value s + s^2 / 2 along +-n and two zeros"""
    n = np.array([2.0, -3.0, 6.0]) / 7.0
    G = (s * np.outer(n, n)).astype(F32)
    e = tensors_of_gradients(np.broadcast_to(G, (1, 3, 3)))
    got = {k: float(v[0]) for k, v in principal_of_tensor(e).items()}
    lam = s + s * s / 2
    big, small, d = ("e1", "e3", "d1") if s > 0 else ("e3", "e1", "d3")
    assert abs(got[big] - lam) <= BOUND["eigenvalue"] * abs(lam)
    assert abs(got["e2"]) <= BOUND["eigenvalue"] * abs(lam) and abs(got[small]) <= BOUND["eigenvalue"] * abs(lam)
    assert abs(got["gmax"] - abs(lam) / 2) <= BOUND["eigenvalue"] * abs(lam)
    want = n if n[np.argmax(np.abs(n))] > 0 else -n       # the sign rule: n_z = 6/7 is the largest component and positive
    vec = np.array([got[d + c] for c in "xyz"])
    # sin of the angle <= |r|_2 / gap (Davis-Kahan) with |r|_2 <= sqrt 3 |r|_inf and gap = |lam| here, plus the error of the norm
    assert np.abs(vec - want).max() <= 2 * BOUND["residual"] + BOUND["orthonormal"], (vec, want)


@pytest.mark.parametrize("shape", [(48, 48, 48), (64, 40, 24)])
def test_a_rigid_rotation_has_no_principal_strain(shape):
    R = rotation(10.0, 10.0)
    x, y, z = grid(shape)
    ctr = [(n - 1) / 2 for n in (shape[2], shape[1], shape[0])]
    p = [x - ctr[0], y - ctr[1], z - ctr[2]]
    d = [sum((R[r][c] - (r == c)) * p[c] for c in range(3)).astype(F32) for r in range(3)]
    got = principal_ref(*d)
    for n in ("e1", "e2", "e3", "gmax"):
        assert not np.isnan(got[n]).any()
        assert float(np.abs(got[n]).max()) < 1e-5, (n, float(np.abs(got[n]).max()))   # the bound of the strain fields' own test


def test_the_sign_rule():
    """the component of largest magnitude is non-negative, the first one among equals deciding"""
    rng = np.random.default_rng(9)
    G = rng.uniform(-0.3, 0.3, size=(20000, 3, 3)).astype(F32)
    got = principal_of_tensor(tensors_of_gradients(G))
    for d in ("d1", "d3"):
        v = np.stack([got[d + c] for c in "xyz"], -1)
        lead = v[np.arange(len(v)), np.argmax(np.abs(v), axis=1)]       # argmax takes the first of equals
        assert (lead > 0).all()
    # a 45 degree shear in the x-y plane: d = (1, +-1, 0) / sqrt 2, |x| = |y|, so x decides
    e = tuple(np.array([v], F32) for v in (0, 0, 0, 0.125, 0, 0))
    got = principal_of_tensor(e)
    assert got["d1x"][0] > 0 and got["d3x"][0] > 0 and got["d1y"][0] > 0 and got["d3y"][0] < 0
    assert got["e1"][0] == F32(0.125) and got["e3"][0] == F32(-0.125) and got["e2"][0] == 0


# ---- missing samples ---------------------------------------------------------------------------------------------------------------

def test_the_undefined_set_is_that_of_the_strain_fields():
    dims = (37, 21, 9)
    rng = np.random.default_rng(12)
    comps = X.smooth_displacement(dims, "sine", amp=0.2, seed=5)
    all_nan, one_nan = X.seam_holes(dims, rng, density=0.05)
    comps = X.with_holes(comps, all_nan, one_nan, which=2)
    got = principal_ref(*comps)
    und = np.isnan(strain_ref(*comps)["exx"])
    assert und.any() and not und.all()
    assert np.array_equal(und, X.predicted_undefined(all_nan | one_nan))
    for n in NAMES:
        assert np.array_equal(np.isnan(got[n]), und), n
    st = principal_stats_ref(got["e1"], got["e3"], got["gmax"])
    assert st["defined"] == int((~und).sum())
    assert st["e1_max"] == float(np.nanmax(got["e1"])) and st["e3_min"] == float(np.nanmin(got["e3"]))
    none = principal_stats_ref(*(np.full((2, 2, 2), np.nan, F32),) * 3)
    assert none["defined"] == 0 and all(np.isnan(none[k]) for k in ("e1_max", "e3_min", "shear_max"))


@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 1, 9), (1, 1, 1), (2, 5, 1)])
def test_an_axis_of_size_one(shape):
    """its column of G is 0, nothing is undefined; a single voxel has no strain at all"""
    rng = np.random.default_rng(sum(shape))
    d = [rng.uniform(-1, 1, size=shape).astype(F32) for _ in range(3)]
    got = principal_ref(*d)
    assert not any(np.isnan(got[n]).any() for n in NAMES)
    if shape == (1, 1, 1):
        assert not got["e1"].any() and not got["e3"].any() and got["d1x"][0, 0, 0] == 1 and got["d3z"][0, 0, 0] == 1


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
    for call in (lambda: flow.principal("flow"), lambda: flow.principal("flow", fields=("dir1",)),
                 lambda: pkg.principal_strain(u, v, w)):
        try:
            call(); raise SystemExit("a principal strain call succeeded without f3d_principal_strain")
        except pkg.F3dError as e:
            assert "f3d_principal_strain" in str(e), str(e)
    # the C API itself, without the binding in between
    host = pkg.host()
    ptrs = (pkg._fp * 10)(*[np.empty((D, H, W), np.float32).ctypes.data_as(pkg._fp) for _ in range(10)])
    assert host.f3d_flow_principal_compute(flow._h, 0, 15, ptrs, None) != 0
    assert b"f3d_principal_strain" in host.f3d_host_last_error()
    try:
        flow.principal("trajectory"); raise SystemExit("principal strains of a trajectory that was never started succeeded")
    except pkg.F3dError as e:
        assert "trajectory" in str(e), str(e)
    flow.principal_end()
    assert all(np.array_equal(a, b) for a, b in zip(flow.download(), (u, v, w)))   # the driver still holds its flow
    flow.destroy()
    print("ok weak")
''')


def test_the_host_library_loads_without_the_device_entry():
    """tests/cpu_device does not define f3d_principal_strain: libf3d_host.so built against it must still load (RTLD_NOW) and solve,
    and principal_strain, OpticalFlow.principal and f3d_flow_principal_compute must fail with a message naming the missing entry"""
    subprocess.run(["make", "-C", CPU, "all", "-j4"], check=True, stdout=subprocess.DEVNULL)
    libdir = os.path.join(CPU, "_build", "plain")
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, "libf3d_hip.so")], capture_output=True, text=True).stdout
    assert "f3d_principal_strain" not in names
    env = dict(os.environ, F3D_ROOT=ROOT, F3D_TEST_LIBDIR=libdir, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-c", CASE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok weak" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


# ---- flow3d --principal ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,needle", [(["--principal", "val,strain"], "usage"), (["--principal", ""], "usage"),
                                          (["--principal", "val,,shear"], "usage"), (["--principal"], "usage"),
                                          (["--principal", "e"], "usage"), (["--strain", "vol", "--principal", "dir2"], "usage"),
                                          (["--principal", "val", "--partial"], "--principal"),
                                          (["--principal", "dir1,dir3", "--concurrent", "2"], "--principal")])
def test_flow3d_principal_argument_errors(tmp_path, extra, needle):
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
    assert needle in run.stdout and "usage" in run.stdout
    assert not any("principal" in n or "strain" in n or "flow-" in n for n in os.listdir(tmp_path))


# ---- the headers -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("header,lib,names", [("f3d.h", "hip", ["f3d_principal_strain"]),
                                              ("f3d_host.h", "host", ["f3d_flow_principal_compute", "f3d_flow_principal_end"])])
def test_the_new_entries_are_declared_and_exported(f3d, header, lib, names):
    from test_abi import declared
    handle = getattr(f3d, lib)()
    have = declared(header)
    for n in names:
        assert n in have and hasattr(handle, n), n
    assert not [n for n in have if not hasattr(handle, n)]


def test_the_binding_names_the_outputs_in_abi_order(f3d):
    assert f3d.PRINCIPAL_NAMES == NAMES
    assert f3d.PRINCIPAL_GROUPS == {"val": 1, "shear": 2, "dir1": 4, "dir3": 8}
    assert f3d._principal_mask("val,dir3") == 9 and f3d._principal_mask(("shear",)) == 2
    for bad in ("", "val,", "e", ()):
        with pytest.raises(ValueError):
            f3d._principal_mask(bad)
    import ctypes as C
    assert C.sizeof(f3d.PrincipalStats) == 24
