"""Every derived-field and labelled-body launch past 2 GiB and past 4 GiB of a container: the entries added since the reference's six
operators, through the C ABI on views of the 5 GiB rig of tests/wide_container.py.  A 70 x 20 box in the corner of a container whose
planes are hundreds of MiB forms the byte offsets of a 1024^3 volume with a few ten thousand voxels of work.

Two geometries over the same allocation.  A: planes of 256 MiB (8192 rows) and a box of 19 planes; planes 8 and up lie past 2 GiB of a
view, planes 16 to 18 past 4 GiB.  B: planes of 128 MiB (4096 rows) and a box of 39 planes, for every entry whose workgroup marches a
tile of kZ = 32 planes: one workgroup's own march crosses 2 GiB at plane 16 and 4 GiB at plane 32, and the z-tile seam 31|32 lies on
the 4 GiB line.

Every case asserts, in this order:
 * its premises, from the geometry alone;
 * the same box through the same entry in a dense container (W + 3, H + 2, D + 1) and in the views of the rig give the same words:
   outputs, host tables, statistics (a result does not depend on the container's geometry);
 * Views.check(): outputs, the margin of MX columns and MY rows and the plane on either side, the strip behind every output and
   every input hold what they must;
 * the result equals the plain restatement the entry's own GPU test uses, under that test's bound: the references, the comparison
   functions and the bounds are imported from those modules, none is restated here.

Padding: what the entry's own test pads with -- NaN for interpolated and differentiated fields (a NaN that was read shows), a finite
sentinel for the median test, a FOREGROUND value for thresholded volumes, seeds for the distance transform, a body's label or -1
(foreign) for label volumes.  The sentinel-filled host tables have three rows more than are handed out; those must survive.

The module sorts behind tests/test_gpu_pipeline.py, page-locks nothing, builds no host block above 0.66 MB and keeps its tables at a
few thousand rows (LABBOOK.md)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import wide_container as wc

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 70, 20
# name -> (container height, container planes, planes of the box)
GEOMETRY = {"A": (8192, 20, 19), "B": (4096, 40, 39)}
SENTINEL = 0x7F
WORD = 0x7F7F7F7F            # a finite float (3.39e38), a label far outside every n_labels
ROWS_MORE = 3                # sentinel rows behind the handed-out part of every host table
FOREGROUND = 0x3F3F3F3F      # 0.747: inside [0.5, 1]
SEED = 0x01010101            # a seed of mode "nonzero"
IN_RANGE = 0x42424242        # 48.56: inside every range of bins used here


@pytest.fixture(scope="module")
def rigs(f3d):
    free, _ = f3d.mem_info()
    if free < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free (%.1f GiB)" % (free / 2.0 ** 30))
    r = wc.Rigs(f3d)
    yield r
    r.close()


# ---- the two containers of a case ---------------------------------------------------------------------------------------------------------

def padded(vol, word=wc.FILL):
    """the box with its margin (MX columns, MY rows, one plane) holding `word`: what is uploaded, to both containers"""
    vol = np.ascontiguousarray(vol, F32)
    d, h, w = vol.shape
    full = np.full((d + 1, h + wc.MY, w + wc.MX), word, np.uint32).view(F32)
    full[:d, :h, :w] = vol
    return full


def as_float(labels):
    return np.ascontiguousarray(labels, np.int32).view(F32)


class WideBox:
    """views of the rig: every input and output has its host image (wc.Views), every output an untouched strip behind it"""

    def __init__(self, rig, dims):
        self.rig, self.dims = rig, dims
        self.views = wc.Views(rig, dims)

    def use(self):
        self.rig.cont.set_current()

    def put(self, full):
        return self.views.new(full)

    def out(self):
        return self.views.new(guard=True)

    def get(self, p):
        w, h, d = self.dims
        return self.rig.download(p, w, h, (0, d))


class DenseBox:
    """containers three columns, two rows and a plane larger than the box, as the entries' own tests use"""

    def __init__(self, f3d, dims):
        w, h, d = dims
        self.dims, self.cdims = dims, (w + wc.MX, h + wc.MY, d + 1)
        self.cont = f3d.Containers(*self.cdims)
        self.outs = []

    def use(self):
        self.cont.set_current()

    def put(self, full):
        p = self.cont.alloc(fill=0xFF)
        self.cont.upload(p, full)
        return p

    def out(self):
        self.outs.append(self.cont.alloc(fill=0xFF))
        return self.outs[-1]

    def get(self, p):
        return self.cont.download(p, self.dims)

    def margins_hold_the_fill(self):
        w, h, d = self.dims
        outside = np.ones(self.cdims[::-1], bool)
        outside[:d, :h, :w] = False
        return all(bool((wc.words(self.cont.download(p, self.cdims))[outside] == wc.FILL).all()) for p in self.outs)

    def free(self):
        self.cont.free()


def raw(value):
    """the bytes of a host result: ctypes structures and arrays, numpy arrays, plain numbers"""
    if isinstance(value, np.ndarray):
        return value.tobytes()
    if isinstance(value, (C.Structure, C.Array, C._SimpleCData)):
        return bytes(value)
    return repr(value).encode()


def table(ctype, rows):
    """`rows` + ROWS_MORE structures filled with the sentinel byte"""
    t = (ctype * (rows + ROWS_MORE))()
    C.memset(t, SENTINEL, C.sizeof(t))
    return t


def tail_survives(t, rows):
    tail = np.frombuffer(t, np.uint8)[rows * C.sizeof(t._type_):]
    return tail.size == ROWS_MORE * C.sizeof(t._type_) and bool((tail == SENTINEL).all())


def assert_premises(rig, dims, geometry, what):
    """from the geometry alone: the last plane of the box lies at 2^32 bytes or more from its view's base, some plane between 2^31 and
    2^32; in geometry B the z-tile seam 31|32 of a march of 32 planes lies on the 4 GiB line.  -> first plane past 4 GiB"""
    hc, dc, depth = GEOMETRY[geometry]
    assert dims == (W, H, depth) and rig.hc == hc and rig.dc == dc and rig.plane_bytes == hc * wc.PITCH
    offsets = [z * rig.plane_bytes for z in range(depth)]
    assert offsets[-1] >= 1 << 32, f"{what}: the last plane lies at {offsets[-1]} bytes"
    between = [z for z, o in enumerate(offsets) if 1 << 31 <= o < 1 << 32]
    assert between, f"{what}: no plane between 2 GiB and 4 GiB"
    past = (1 << 32) // rig.plane_bytes
    if geometry == "B":
        assert past == 32 and 32 * rig.plane_bytes == 1 << 32 and depth > 32
    assert (hc // (H + wc.MY)) >= 60, "room for the views of the largest case"
    print(f"{what}: geometry {geometry}, box {dims}, planes of {rig.plane_bytes >> 20} MiB: planes {between[0]} .. {between[-1]} lie between "
          f"2 GiB and 4 GiB of a view, planes {past} .. {depth - 1} past 4 GiB; the last at {offsets[-1]} bytes")
    return past


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------

def grid(depth):
    return np.meshgrid(np.arange(depth), np.arange(H), np.arange(W), indexing="ij")


def past_4_gib(depth):
    return {19: 16, 39: 32}[depth]


@functools.lru_cache(maxsize=None)
def bodies(depth, holes=True):
    """(volume, labels, sizes, info): a thresholded volume whose bodies are columns seven voxels wide that wander one voxel in x from
    plane to plane and span every plane of the box (so each lies on both sides of the 2 GiB and the 4 GiB line), cut by a wall at
    y = 9 for x < 35, with random holes (a wrong plane or row changes the answer), and one body confined past the 4 GiB line;
    labels: components_ref's numbering of it"""
    import components_ref as cref
    z, y, x = grid(depth)
    mask = (x + z % 2) % 10 < 7
    mask &= ~((y == 9) & (x < 35))
    if holes:
        mask &= np.random.default_rng(depth).random(mask.shape) >= 0.08
    p = past_4_gib(depth)
    mask[p:, 13:, 57:] = False
    mask[p + 1:, 15:19, 60:68] = True
    volume = cref.as_volume(mask, 0.75, 0.25)
    labels, sizes, info = cref.label_components(volume, 0.5, 1.0, 1)
    for a in (volume, labels, sizes):
        a.setflags(write=False)
    return volume, labels, sizes, info


def assert_bodies(labels, n_labels, depth):
    """several bodies on both sides of plane 16 (and of plane 32 in geometry B), one confined past the 4 GiB line"""
    p = past_4_gib(depth)
    z = grid(depth)[0]
    first = np.full(n_labels + 1, depth)
    last = np.full(n_labels + 1, -1)
    body = (labels >= 1) & (labels <= n_labels)
    np.minimum.at(first, labels[body], z[body])
    np.maximum.at(last, labels[body], z[body])
    for line in {16, p}:
        assert int(((first[1:] < line) & (last[1:] >= line)).sum()) >= 5, f"bodies across plane {line}"
    assert int(((first[1:] >= p) & (last[1:] >= first[1:])).sum()) >= 1, "a body confined past the 4 GiB line"


@functools.lru_cache(maxsize=None)
def segmentation(depth):
    """(labels, n_labels): fourteen TOUCHING bodies, slabs ten voxels wide that wander one voxel in x from plane to plane and span every
    plane of the box, a fifteenth confined past the 4 GiB line, 8 % background and 2 % foreign voxels (negative, and one past n_labels)"""
    z, y, x = grid(depth)
    lab = (1 + (x + z % 2) // 10 % 7 + 7 * (y >= 10)).astype(np.int32)
    n = 15
    p = past_4_gib(depth)
    lab[p + 1:, 15:19, 60:68] = n
    pick = np.random.default_rng(depth + 1).random(lab.shape)
    lab[pick < 0.08] = 0
    lab[(pick >= 0.08) & (pick < 0.09)] = -3
    lab[(pick >= 0.09) & (pick < 0.10)] = n + 1
    assert_bodies(lab, n, depth)
    lab.setflags(write=False)
    return lab, n


def gather_displacement(depth, seed, holes=0.01):
    """a few voxels along z, so that the corners of a gather lie across the 2 GiB and 4 GiB lines"""
    rng = np.random.default_rng(seed)
    u, v = (rng.uniform(-2, 2, (depth, H, W)).astype(F32) for _ in range(2))
    w = rng.uniform(-4, 4, (depth, H, W)).astype(F32)
    u[rng.random(u.shape) < holes] = np.nan
    return u, v, w


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def same_words(got, want):
    return got.shape == want.shape and bool((wc.words(got) == wc.words(want)).all())


# ---- the cases: inputs (once), one launch into a box, the comparison with the restatement ---------------------------------------------------

class Case:
    entries, geometry = (), "B"

    @classmethod
    def dims(cls):
        return (W, H, GEOMETRY[cls.geometry][2])

    @classmethod
    @functools.lru_cache(maxsize=None)
    def given(cls):
        """inputs and the restatement's result, computed once and left unchanged"""
        return cls.make(cls.dims())


class ComposeFlow(Case):
    entries, geometry = ("f3d_compose_flow",), "A"

    @staticmethod
    def make(dims):
        from test_gpu_trajectory import random_step
        from trajectory_ref import compose_ref
        acc, inc = random_step(np.random.default_rng(1), *dims)
        acc[2] += np.random.default_rng(2).uniform(-3, 3, acc[2].shape).astype(F32)          # a few voxels along z
        want = compose_ref(acc, inc)
        return frozen(*acc), frozen(*inc), frozen(*want)

    @staticmethod
    def launch(f3d, box, given):
        acc, inc, _ = given
        pa, pi = [box.put(padded(a)) for a in acc], [box.put(padded(a)) for a in inc]
        box.use()
        lost = C.c_ulonglong()
        f3d.check(f3d._compose_entry()(*pa, *pi, *ComposeFlow.dims(), C.byref(lost)), "f3d_compose_flow")
        return dict(zip("uvw", pa)), {"lost": lost}

    @staticmethod
    def verify(f3d, given, out, host):
        from trajectory_ref import same_bits
        want = given[2]
        for n, e in zip("uvw", want):
            assert same_bits(out[n], e), f"f3d_compose_flow {n}"
        lost = int(np.isnan(want[0]).sum())
        assert host["lost"].value == lost and 0 < lost < want[0].size


class InitialFlow(Case):
    entries, geometry = ("f3d_initial_flow",), "A"

    @staticmethod
    def make(dims):
        import warm_start_ref as ws
        w, h, d = dims
        rng = np.random.default_rng(28)
        guess = [rng.uniform(-3, 3, (d, h, w)).astype(F32) for _ in range(3)]
        pick = rng.random((d, h, w))
        guess[0][pick < 0.02] = np.nan
        guess[1][(pick >= 0.02) & (pick < 0.03)] = np.inf
        guess[2][(pick >= 0.03) & (pick < 0.04)] = -np.inf
        guess[2][(pick >= 0.04) & (pick < 0.10)] *= F32(4)                                    # some end points leave through z
        want, info = ws.initial_flow(*guess)
        assert info["replaced"] > 0 and info["leaving"] > 0
        return frozen(*guess), frozen(*want), info

    @staticmethod
    def launch(f3d, box, given):
        ins = [box.put(padded(a)) for a in given[0]]
        outs = [box.out() for _ in range(3)]
        box.use()
        info = f3d.InitialInfo()
        f3d.check(f3d._initial_entry()(*ins, *outs, *InitialFlow.dims(), C.byref(info)), "f3d_initial_flow")
        return dict(zip("uvw", outs)), {"info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        _, want, info = given
        for n, e in zip("uvw", want):
            assert same_words(out[n], e), f"f3d_initial_flow {n}"
        assert host["info"].as_dict() == info
        assert wc.words(F32(host["info"].max_abs)) == wc.words(F32(info["max_abs"]))


class InvertDisplacement(Case):
    entries, geometry = ("f3d_invert_displacement",), "A"
    ITERATIONS, TOLERANCE = 32, 1e-3

    @staticmethod
    def make(dims):
        from inverse_ref import invert_ref
        w, h, d = dims
        rng = np.random.default_rng(3)
        comps = [rng.uniform(-0.3, 0.3, (d, h, w)).astype(F32) for _ in range(3)]
        comps[2] += F32(2.5)                                                                  # g is about -2.5 planes: gathers across the lines
        comps[1][rng.random((d, h, w)) < 0.01] = np.nan
        want = invert_ref(*comps, iterations=InvertDisplacement.ITERATIONS, tolerance=InvertDisplacement.TOLERANCE)
        return frozen(*comps), frozen(*want)

    @staticmethod
    def launch(f3d, box, given):
        ins = [box.put(padded(a)) for a in given[0]]
        outs = [box.out() for _ in range(4)]
        box.use()
        stats = f3d.InverseStats()
        f3d.check(f3d._inverse_entry()(*ins, *outs, *InvertDisplacement.dims(), InvertDisplacement.ITERATIONS, InvertDisplacement.TOLERANCE,
                                       C.byref(stats)), "f3d_invert_displacement")
        return dict(zip(("gu", "gv", "gw", "err"), outs)), {"stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_inverse import NAMES, check_result
        want = given[1]
        st = check_result([out[n] for n in NAMES] + [host["stats"].as_dict()], want, InvertDisplacement.TOLERANCE, "f3d_invert_displacement")
        assert 0 < st["defined"] < want[0].size


class CarryField(Case):
    entries, geometry = ("f3d_carry_field",), "A"
    MODES = {"linear": 1, "nearest": 2}

    @staticmethod
    def make(dims):
        from inverse_ref import carry_ref
        w, h, d = dims
        rng = np.random.default_rng(4)
        field = rng.integers(0, 9, (d, h, w)).astype(F32)
        field[rng.random((d, h, w)) < 0.01] = np.nan
        m = gather_displacement(d, 5)
        want = {mode: carry_ref(field, *m, mode) for mode in CarryField.MODES}
        return frozen(field, *m), want

    @staticmethod
    def launch(f3d, box, given):
        ins = [box.put(padded(a)) for a in given[0]]
        out, host = {}, {}
        box.use()
        for mode, m in CarryField.MODES.items():
            out[mode], host[mode] = box.out(), C.c_ulonglong()
            f3d.check(f3d._carry_entry()(*ins, out[mode], *CarryField.dims(), m, C.byref(host[mode])), "f3d_carry_field")
        return out, host

    @staticmethod
    def verify(f3d, given, out, host):
        from inverse_ref import same_bits
        for mode, (ref, lost) in given[1].items():
            assert same_bits(out[mode], ref), f"f3d_carry_field {mode}"
            assert host[mode].value == lost and 0 < lost < ref.size


class Grouped(Case):
    """u, v, w -> the outputs of every group and the statistics: f3d_flow_strain, f3d_principal_strain, f3d_polar_decomposition"""

    @classmethod
    def launch(cls, f3d, box, given):
        names = importlib.import_module(cls.REF).NAMES                      # the outputs in ABI order
        ins = [box.put(padded(a)) for a in given[0]]
        outs = [box.out() for _ in names]
        box.use()
        stats = getattr(f3d, cls.STATS)()
        f3d.check(getattr(f3d, cls.ENTRY)()(*ins, (f3d._dp * len(outs))(*outs), cls.ALL, *cls.dims(), C.byref(stats)), cls.entries[0])
        return dict(zip(names, outs)), {"stats": stats}


class FlowStrain(Grouped):
    entries, ALL = ("f3d_flow_strain",), 7
    REF, ENTRY, STATS = "strain_ref", "_strain_entry", "StrainStats"

    @staticmethod
    def make(dims):
        from strain_ref import strain_ref
        from test_gpu_strain import random_displacement
        comps = random_displacement(np.random.default_rng(6), *dims)
        return frozen(*comps), strain_ref(*comps)

    @staticmethod
    def verify(f3d, given, out, host):
        from strain_ref import NAMES, same_bits
        from test_gpu_strain import check_stats
        want = given[1]
        for n in NAMES:
            assert same_bits(out[n], want[n]), f"f3d_flow_strain {n}"
        check_stats(host["stats"].as_dict(), want["vol"], want["eq"])
        assert 0 < host["stats"].defined < want["vol"].size and host["stats"].folded > 0


class PrincipalStrain(Grouped):
    entries, ALL = ("f3d_principal_strain",), 15
    REF, ENTRY, STATS = "principal_ref", "_principal_entry", "PrincipalStats"

    @staticmethod
    def make(dims):
        from principal_ref import principal_ref
        from test_gpu_strain import random_displacement
        comps = [c * F32(0.5) for c in random_displacement(np.random.default_rng(7), *dims)]
        return frozen(*comps), principal_ref(*comps)

    @staticmethod
    def verify(f3d, given, out, host):
        from principal_ref import NAMES
        from strain_ref import same_bits
        from test_gpu_principal import check_stats
        want = given[1]
        for n in NAMES:
            assert same_bits(out[n], want[n]), f"f3d_principal_strain {n}"
        check_stats(host["stats"].as_dict(), want)
        assert 0 < host["stats"].defined < want["e1"].size


class PolarDecomposition(Grouped):
    entries, ALL = ("f3d_polar_decomposition",), 7
    REF, ENTRY, STATS = "polar_ref", "_polar_entry", "PolarStats"

    @staticmethod
    def make(dims):
        from polar_ref import polar_ref
        from test_gpu_polar import displacement
        comps = displacement("rotated", dims)
        return frozen(*comps), polar_ref(*comps)

    @staticmethod
    def verify(f3d, given, out, host):
        from polar_ref import NAMES
        from strain_ref import same_bits
        from test_gpu_polar import check_stats
        want, folded = given[1]
        for n in NAMES:
            assert same_bits(out[n], want[n]), f"f3d_polar_decomposition {n}"
        st = check_stats(host["stats"].as_dict(), want, folded)
        assert 0 < st["defined"] < want["theta"].size


class WindowStrain(Case):
    entries = ("f3d_window_strain",)
    RADIUS, MIN_COUNT, ALL = 2, 4, 15

    @staticmethod
    def make(dims):
        from test_gpu_window_strain import displacement
        from window_strain_ref import window_strain_ref
        comps = displacement(np.random.default_rng(8), *dims, WindowStrain.RADIUS)
        return frozen(*comps), window_strain_ref(*comps, WindowStrain.RADIUS, WindowStrain.MIN_COUNT)

    @staticmethod
    def launch(f3d, box, given):
        from window_strain_ref import NAMES
        ins = [box.put(padded(a)) for a in given[0]]
        outs = [box.out() for _ in NAMES]
        box.use()
        stats = f3d.WindowStrainStats()
        f3d.check(f3d._window_strain_entry()(*ins, (f3d._dp * len(outs))(*outs), WindowStrain.ALL, WindowStrain.RADIUS, WindowStrain.MIN_COUNT,
                                             *WindowStrain.dims(), C.byref(stats)), "f3d_window_strain")
        return dict(zip(NAMES, outs)), {"stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_window_strain import check_stats
        from window_strain_ref import NAMES, same_bits
        want, want_stats = given[1]
        for n in NAMES:
            assert same_bits(out[n], want[n]), f"f3d_window_strain {n}"
        st = host["stats"].as_dict()
        check_stats(st, want_stats)
        assert st["defined"] > want["vol"].size // 2 and st["lost"] > 0


class FromGradient(Case):
    """nine stored gradient entries -> f3d_principal_from_gradient and f3d_polar_from_gradient"""
    entries = ("f3d_principal_from_gradient", "f3d_polar_from_gradient")

    @staticmethod
    def make(dims):
        from test_gpu_from_gradient import KINDS, gradient, reference
        grad = gradient("nan", dims, np.random.default_rng(9))
        return frozen(*grad), {kind: reference(kind, grad) for kind in KINDS}

    @staticmethod
    def launch(f3d, box, given):
        from test_gpu_from_gradient import KINDS
        ins = [box.put(padded(a)) for a in given[0]]
        out, host = {}, {}
        box.use()
        for kind, K in KINDS.items():
            fn = f3d._principal_from_gradient_entry() if kind == "principal" else f3d._polar_from_gradient_entry()
            outs = [box.out() for _ in K["names"]]
            host[kind] = (f3d.PrincipalStats if kind == "principal" else f3d.PolarStats)()
            f3d.check(fn((f3d._dp * 9)(*ins), (f3d._dp * len(outs))(*outs), K["all"], *FromGradient.dims(), C.byref(host[kind])),
                      f"f3d_{kind}_from_gradient")
            out.update({f"{kind}/{n}": p for n, p in zip(K["names"], outs)})
        return out, host

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_from_gradient import KINDS, check_fields, check_stats
        for kind, K in KINDS.items():
            want, want_stats = given[1][kind]
            check_fields({n: out[f"{kind}/{n}"] for n in K["names"]}, want, K["names"], f"f3d_{kind}_from_gradient")
            check_stats(host[kind].as_dict(), want_stats, f"f3d_{kind}_from_gradient")
            assert 0 < want_stats["defined"] < given[0][0].size


class LocalCorrelation(Case):
    entries = ("f3d_local_correlation",)
    RADIUS = 3

    @staticmethod
    def make(dims):
        from correlation_ref import local_correlation
        from test_gpu_correlation import THRESHOLD, pair_of_volumes
        a, b = pair_of_volumes(np.random.default_rng(10), *dims)
        return frozen(a, b), local_correlation(a, b, LocalCorrelation.RADIUS, THRESHOLD)

    @staticmethod
    def launch(f3d, box, given):
        from test_gpu_correlation import THRESHOLD
        ins = [box.put(padded(a)) for a in given[0]]
        outs = [box.out() for _ in range(2)]
        box.use()
        stats = f3d.CorrelationStats()
        f3d.check(f3d._correlation_entry()(*ins, (f3d._dp * 2)(*outs), 3, LocalCorrelation.RADIUS, THRESHOLD, *LocalCorrelation.dims(),
                                           C.byref(stats)), "f3d_local_correlation")
        return dict(zip(("zncc", "rmsd"), outs)), {"stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from correlation_ref import same_bits
        from test_gpu_correlation import check_stats
        zncc, rmsd, want = given[1]
        assert same_bits(out["zncc"], zncc) and same_bits(out["rmsd"], rmsd)
        st = host["stats"].as_dict()
        check_stats(st, want)
        assert 0 < st["defined"] < zncc.size and st["lost"] > 0 and st["below"] > 0


class Motion(Case):
    entries = ("f3d_motion_sums", "f3d_remove_motion")

    @staticmethod
    def fit(dims):
        """test_gpu_motion.make_fit's "large" fit as plain lists (centre, t, M)"""
        from test_gpu_motion import make_fit
        fit = make_fit(importlib.import_module("cuda-flow3d_amd"), dims, "large")
        return list(fit.centre), list(fit.t), list(fit.M)

    @staticmethod
    def make(dims):
        import motion_ref as ref
        from test_gpu_motion import WEIGHT_MIN, case_inputs
        u, v, w, weight = case_inputs(dims, "weight")
        hu, hv, hw, _ = case_inputs(dims, "holes")
        return (frozen(u, v, w, weight), frozen(hu, hv, hw), ref.motion_sums(u, v, w, weight, WEIGHT_MIN),
                ref.remove_motion(hu, hv, hw, *Motion.fit(dims)))

    @staticmethod
    def launch(f3d, box, given):
        from test_gpu_motion import WEIGHT_MIN
        sums_fn, remove_fn = f3d._motion_entry()
        ins = [box.put(padded(a)) for a in given[0]]
        holes = [box.put(padded(a)) for a in given[1]]
        outs = [box.out() for _ in range(3)]
        box.use()
        sums, stats, fit = f3d.MotionSums(), f3d.MotionResidual(), f3d.MotionFit()
        fit.centre[:], fit.t[:], fit.M[:] = Motion.fit(Motion.dims())
        f3d.check(sums_fn(*ins, WEIGHT_MIN, *Motion.dims(), C.byref(sums)), "f3d_motion_sums")
        f3d.check(remove_fn(*holes, *outs, C.byref(fit), *Motion.dims(), C.byref(stats)), "f3d_remove_motion")
        return dict(zip("uvw", outs)), {"sums": sums, "stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_motion import check_residual_stats, check_sums
        check_sums(host["sums"], given[2])
        assert 0 < host["sums"].n < given[0][0].size
        want = given[3]
        for n, e in zip("uvw", want):
            assert same_words(out[n], e), f"f3d_remove_motion {n}"
        check_residual_stats(host["stats"].as_dict(), want[3])


class LabelMotion(Case):
    entries = ("f3d_label_motion_sums", "f3d_remove_label_motion")

    @staticmethod
    def fits(dims, n):
        from test_gpu_label_motion import make_fits
        return make_fits(importlib.import_module("cuda-flow3d_amd"), dims, n)

    @staticmethod
    def make(dims):
        import label_motion_ref as ref
        from test_gpu_label_motion import WEIGHT_MIN, fit_arrays, values
        labels, n = segmentation(dims[2])
        u, v, w, weight = values(dims, True)
        rng = np.random.default_rng(11)
        noise = [rng.normal(m, 1.5, labels.shape).astype(F32) for m in (2.0, -1.0, 0.5)]
        noise[0][rng.random(labels.shape) < 0.04] = np.nan
        return (frozen(u, v, w, weight), frozen(*noise), ref.label_sums(u, v, w, labels, n, weight, WEIGHT_MIN),
                ref.remove_label_motion(*noise, labels, *fit_arrays(*LabelMotion.fits(dims, n))))

    @staticmethod
    def launch(f3d, box, given):
        from test_gpu_label_motion import WEIGHT_MIN
        dims = LabelMotion.dims()
        labels, n = segmentation(dims[2])
        sums_fn, remove_fn = f3d._label_motion_entry()
        u, v, w, weight = [box.put(padded(a)) for a in given[0]]
        noise = [box.put(padded(a)) for a in given[1]]
        pl = box.put(padded(as_float(labels)))                               # the padding is -1: foreign
        outs = [box.out() for _ in range(3)]
        box.use()
        sums, info, stats = table(f3d.MotionSums, n), f3d.LabelInfo(), f3d.MotionResidual()
        fits, status = LabelMotion.fits(dims, n)
        f3d.check(sums_fn(u, v, w, pl, n, weight, WEIGHT_MIN, *dims, sums, C.byref(info)), "f3d_label_motion_sums")
        f3d.check(remove_fn(*noise, pl, n, fits, status, *outs, *dims, C.byref(stats)), "f3d_remove_label_motion")
        return dict(zip("uvw", outs)), {"sums": sums, "info": info, "stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_label_motion import check_sums
        from test_gpu_motion import check_residual_stats
        _, n = segmentation(LabelMotion.dims()[2])
        want, info = given[2]
        check_sums(list(host["sums"])[:n], want)
        assert tail_survives(host["sums"], n)
        assert host["info"].as_dict() == info and info["foreign"] > 0 and info["used"] > 0
        removed = given[3]
        for c, e in zip("uvw", removed):
            assert same_words(out[c], e), f"f3d_remove_label_motion {c}"
        check_residual_stats(host["stats"].as_dict(), removed[3])


class LabelContacts(Case):
    entries = ("f3d_label_contacts",)

    @staticmethod
    def make(dims):
        import contacts_ref as ref
        from test_gpu_label_motion import values
        labels, n = segmentation(dims[2])
        u, v, w = values(dims, False)[:3]
        want, info = ref.label_contacts(u, v, w, labels, n)
        assert 8 <= len(want) <= 4000
        return frozen(u, v, w), want, info

    @staticmethod
    def launch(f3d, box, given):
        dims = LabelContacts.dims()
        labels, n = segmentation(dims[2])
        ins = [box.put(padded(a)) for a in given[0]]
        pl = box.put(padded(as_float(labels)))                               # the padding is -1: a read past the box shows as foreign faces
        box.use()
        rows, info = table(f3d.Contact, len(given[1])), f3d.ContactInfo()
        f3d.check(f3d._contacts_entry()(*ins, pl, n, *dims, len(given[1]), rows, C.byref(info)), "f3d_label_contacts")
        return {}, {"rows": rows, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_contacts import check_info, check_rows
        _, want, info = given
        check_info(host["info"].as_dict(), info, LabelContacts.dims())
        check_rows(list(host["rows"])[:len(want)], want)
        assert tail_survives(host["rows"], len(want))


class LabelComponents(Case):
    entries = ("f3d_label_components",)
    ROOM = 2048

    @staticmethod
    def make(dims):
        volume, labels, sizes, info = bodies(dims[2])
        assert_bodies(labels, int(info["n_labels"]), dims[2])
        return (volume,), (labels, sizes, info)

    @staticmethod
    def launch(f3d, box, given):
        src = box.put(padded(given[0][0], FOREGROUND))                        # a read past the box would join bodies
        dst = box.out()
        box.use()
        sizes = np.full(LabelComponents.ROOM + ROWS_MORE, WORD << 32 | WORD, np.uint64)
        info = f3d.ComponentInfo()
        f3d.check(f3d._components_entry()(src, 0.5, 1.0, 1, dst, *LabelComponents.dims(), sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                          LabelComponents.ROOM, C.byref(info)), "f3d_label_components")
        return {"labels": dst}, {"sizes": sizes, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        labels, sizes, info = given[1]
        n = len(sizes)
        assert n <= LabelComponents.ROOM and host["info"].as_dict() == info
        assert np.array_equal(out["labels"].view(np.int32), labels)
        assert np.array_equal(host["sizes"][:n], sizes) and (host["sizes"][n:] == (WORD << 32 | WORD)).all()


class NearestSeed(Case):
    entries = ("f3d_nearest_seed",)

    @staticmethod
    def make(dims):
        import nearest_ref as ref
        w, h, d = dims
        rng = np.random.default_rng(12)
        values = np.where(rng.random((d, h, w)) < 0.002, rng.integers(1, 1000, (d, h, w)), 0).astype(np.int32)
        z = grid(d)[0]
        assert (values[z < 16] != 0).any() and (values[z >= past_4_gib(d)] != 0).any()
        want = ref.nearest_separable(values, "nonzero")
        assert want[3]["d2_max"] > 9                                          # the nearest seed of many voxels lies across a line
        return frozen(values), frozen(*want[:3]) + (want[3],)

    @staticmethod
    def launch(f3d, box, given):
        import nearest_ref as ref
        src = box.put(padded(as_float(given[0][0]), SEED))                    # a read past the box would shorten distances
        outs = [box.out() for _ in ref.OUTPUTS]
        box.use()
        info = f3d.NearestInfo()
        f3d.check(f3d._nearest_entry()(src, 0, 0, *outs, *NearestSeed.dims(), C.byref(info)), "f3d_nearest_seed")
        return dict(zip(ref.OUTPUTS, outs)), {"info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        import nearest_ref as ref
        want = given[1]
        assert host["info"].as_dict() == want[3]
        for name, e in zip(ref.OUTPUTS, want[:3]):
            assert np.array_equal(out[name].view(np.int32), e), f"f3d_nearest_seed {name}"


class SplitComponents(Case):
    entries = ("f3d_split_components",)
    ROOM, CORE_D2 = 2048, 9

    @staticmethod
    def make(dims):
        import nearest_ref as ref
        volume = bodies(dims[2], holes=False)[0]
        labels, sizes, info = ref.split_components(volume, 0.5, 1.0, SplitComponents.CORE_D2, 1)
        assert info["n_cores"] >= 5 and info["core_voxels"] < info["foreground"]
        return (volume,), frozen(labels, sizes) + (info,)

    @staticmethod
    def launch(f3d, box, given):
        src = box.put(padded(given[0][0], FOREGROUND))
        dst = box.out()
        box.use()
        sizes = np.full(SplitComponents.ROOM + ROWS_MORE, WORD << 32 | WORD, np.uint64)
        info = f3d.SplitInfo()
        f3d.check(f3d._split_entry()(src, 0.5, 1.0, SplitComponents.CORE_D2, 1, dst, *SplitComponents.dims(),
                                     sizes.ctypes.data_as(C.POINTER(C.c_ulonglong)), SplitComponents.ROOM, C.byref(info)), "f3d_split_components")
        return {"labels": dst}, {"sizes": sizes, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        labels, sizes, info = given[1]
        n = len(sizes)
        assert n <= SplitComponents.ROOM and host["info"].as_dict() == info
        assert np.array_equal(out["labels"].view(np.int32), labels)
        assert np.array_equal(host["sizes"][:n], sizes) and (host["sizes"][n:] == (WORD << 32 | WORD)).all()


class LabelShape(Case):
    entries = ("f3d_label_shape_sums",)

    @staticmethod
    def make(dims):
        import label_shape_ref as ref
        labels, n = segmentation(dims[2])
        return (), ref.label_shape_sums(labels, n)

    @staticmethod
    def launch(f3d, box, given):
        dims = LabelShape.dims()
        labels, n = segmentation(dims[2])
        pl = box.put(padded(as_float(labels), 1))                             # the padding carries a body's label
        box.use()
        rows, info = table(f3d.LabelShapeSums, n), f3d.LabelShapeInfo()
        f3d.check(f3d._label_shape_entry()(pl, n, *dims, rows, C.byref(info)), "f3d_label_shape_sums")
        return {}, {"rows": rows, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        import label_shape_ref as ref
        from test_gpu_shape_of_labels import check_sums
        _, n = segmentation(LabelShape.dims()[2])
        want, info = given[1]
        assert host["info"].as_dict() == info
        check_sums(np.frombuffer(host["rows"], ref.SUMS_DTYPE)[:n], want)
        assert tail_survives(host["rows"], n)


class LabelOverlap(Case):
    entries = ("f3d_label_overlap", "f3d_relabel_labels")

    @staticmethod
    def make(dims):
        import overlap_ref as ref
        la, n = segmentation(dims[2])
        lb = np.roll(la, (3, 1, 2), axis=(0, 1, 2))                           # the same bodies three planes on
        u, v, w = gather_displacement(dims[2], 13, holes=0.02)
        rows, info = ref.label_overlap(la, n, lb, n, u, v, w)
        assert 8 <= len(rows) <= 4000 and info["lost_body"] > 0 and info["overlap"] > 0
        mapping = np.random.default_rng(14).integers(0, n // 2, n).astype(np.int32)       # two labels may share a number; some become 0
        return frozen(lb, u, v, w, mapping), rows, info, ref.relabel(lb, mapping)

    @staticmethod
    def launch(f3d, box, given):
        dims = LabelOverlap.dims()
        la, n = segmentation(dims[2])
        lb, u, v, w, mapping = given[0]
        pa, pb = box.put(padded(as_float(la), 1)), box.put(padded(as_float(lb), 1))
        pd = [box.put(padded(a)) for a in (u, v, w)]
        out = box.out()
        box.use()
        n_pairs = len(given[1])
        rows, info, foreign = table(f3d.Overlap, n_pairs), f3d.OverlapInfo(), C.c_ulonglong()
        f3d.check(f3d._overlap_entry()(pa, n, pb, n, *pd, *dims, n_pairs, rows, C.byref(info)), "f3d_label_overlap")
        f3d.check(f3d._relabel_entry()(pb, n, mapping.ctypes.data_as(C.POINTER(C.c_int)), out, *dims, C.byref(foreign)), "f3d_relabel_labels")
        return {"relabelled": out}, {"rows": rows, "info": info, "foreign": foreign}

    @staticmethod
    def verify(f3d, given, out, host):
        import overlap_ref as ref
        from test_gpu_track_overlap import check_rows
        _, want, info, (relabelled, foreign) = given
        assert host["info"].as_dict() == info
        check_rows(np.frombuffer(host["rows"], ref.ROWS_DTYPE)[:len(want)], want)
        assert tail_survives(host["rows"], len(want))
        assert np.array_equal(out["relabelled"].view(np.int32), relabelled) and host["foreign"].value == foreign > 0


class LabelField(Case):
    entries = ("f3d_label_field_sums", "f3d_paint_labels")
    SHIFT, LO, HI, BINS = 14, -500.0, 750.5, 64

    @staticmethod
    def make(dims):
        import label_field_ref as ref
        labels, n = segmentation(dims[2])
        rng = np.random.default_rng(15)
        field = rng.uniform(-600, 800, labels.shape).astype(F32)
        pick = rng.random(labels.shape)
        field[pick < 0.02] = np.nan
        field[(pick >= 0.02) & (pick < 0.04)] = F32(2000.0)                  # beyond 2^24 quanta: out of range
        values = rng.normal(0, 100, n).astype(F32)
        values[::7] = np.nan
        c = LabelField
        rows, counts, info = ref.label_field_sums(field, labels, n, c.SHIFT, c.LO, c.HI, c.BINS)
        assert info["nan"] > 0 and info["out_of_range"] > 0 and info["used"] > 0
        return frozen(field, values), (rows, counts, info), ref.paint_labels(labels, values)

    @staticmethod
    def launch(f3d, box, given):
        c, dims = LabelField, LabelField.dims()
        labels, n = segmentation(dims[2])
        field, values = given[0]
        pf, pl = box.put(padded(field, IN_RANGE)), box.put(padded(as_float(labels), 1))
        out = box.out()
        box.use()
        rows, info = table(f3d.LabelFieldSumsRow, n), f3d.LabelFieldInfo()
        counts = np.full((n + ROWS_MORE, c.BINS), WORD, np.uint32)
        f3d.check(f3d._label_field_entry()(pf, pl, n, c.SHIFT, c.LO, c.HI, c.BINS, *dims, rows, counts.ctypes.data_as(C.POINTER(C.c_uint)),
                                           C.byref(info)), "f3d_label_field_sums")
        f3d.check(f3d._paint_entry()(pl, n, values.ctypes.data_as(C.POINTER(C.c_float)), out, *dims), "f3d_paint_labels")
        return {"painted": out}, {"rows": rows, "counts": counts, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        import label_field_ref as ref
        from test_gpu_stats_of_label_field import check_rows
        _, n = segmentation(LabelField.dims()[2])
        _, (rows, counts, info), painted = given
        assert host["info"].as_dict() == info
        check_rows(np.frombuffer(host["rows"], ref.SUMS_DTYPE)[:n], rows)
        assert tail_survives(host["rows"], n)
        assert np.array_equal(host["counts"][:n], counts) and (host["counts"][n:] == WORD).all()
        assert np.array_equal(wc.words(out["painted"]), painted)


class Histogram(Case):
    entries = ("f3d_value_range", "f3d_histogram")
    LO, HI, BINS = 10.0, 240.0, 256

    @staticmethod
    def make(dims):
        import histogram_ref as ref
        labels, _ = segmentation(dims[2])
        rng = np.random.default_rng(16)
        volume = rng.uniform(0, 255, labels.shape).astype(F32)
        pick = rng.random(labels.shape)
        volume[pick < 0.02] = np.nan
        volume[(pick >= 0.02) & (pick < 0.03)] = np.inf
        mask = np.where(labels > 0, labels, 0).astype(np.int32)
        c = Histogram
        counts, info = ref.histogram(volume, c.LO, c.HI, c.BINS, mask)
        assert all(info[k] > 0 for k in ref.HISTOGRAM_INFO)
        return frozen(volume, mask), (counts, info), ref.value_range(volume, mask)

    @staticmethod
    def launch(f3d, box, given):
        c, dims = Histogram, Histogram.dims()
        volume, mask = given[0]
        src = box.put(padded(volume, IN_RANGE))
        msk = box.put(padded(as_float(mask), WORD))                          # outside the box every mask word lets a voxel through
        box.use()
        lo, hi, found = C.c_float(), C.c_float(), f3d.RangeInfo()
        f3d.check(f3d._value_range_entry()(src, msk, *dims, C.byref(lo), C.byref(hi), C.byref(found)), "f3d_value_range")
        counts, info = np.full(c.BINS + ROWS_MORE, WORD << 32 | WORD, np.uint64), f3d.HistogramInfo()
        f3d.check(f3d._histogram_entry()(src, msk, c.LO, c.HI, c.BINS, *dims, counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)),
                  "f3d_histogram")
        return {}, {"lo": lo, "hi": hi, "found": found, "counts": counts, "info": info}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_segment_histogram import same_range
        _, (counts, info), want_range = given
        bins = Histogram.BINS
        assert same_range((F32(host["lo"].value), F32(host["hi"].value), host["found"].as_dict()), want_range)
        assert host["info"].as_dict() == info
        assert np.array_equal(host["counts"][:bins], counts) and (host["counts"][bins:] == (WORD << 32 | WORD)).all()


class ValidateDisplacement(Case):
    entries = ("f3d_validate_displacement",)
    STEP, THRESHOLD, MIN_NEIGHBOURS = 1, 2.0, 9

    @staticmethod
    def make(dims):
        import outlier_ref as ref
        from test_gpu_outlier import EPS, WEIGHT_MIN, case_inputs
        c = ValidateDisplacement
        u, v, w, weight = case_inputs(dims, "weight")
        want = ref.validate(u, v, w, weight, WEIGHT_MIN, c.STEP, EPS, c.THRESHOLD, c.MIN_NEIGHBOURS, ref.REPLACE)
        assert want[4]["outliers"] > 0 and want[4]["replaced"] > 0
        return frozen(u, v, w, weight), want

    @staticmethod
    def launch(f3d, box, given):
        import outlier_ref as ref
        from test_gpu_outlier import EPS, WEIGHT_MIN
        c = ValidateDisplacement
        u, v, w, weight = [box.put(padded(a, WORD)) for a in given[0]]       # finite: a NaN margin read by mistake would pass for absent
        outs = [box.out() for _ in range(4)]
        box.use()
        stats = f3d.ValidateStats()
        f3d.check(f3d._validate_entry()(u, v, w, weight, WEIGHT_MIN, c.STEP, EPS, c.THRESHOLD, c.MIN_NEIGHBOURS, ref.REPLACE,
                                        (f3d._dp * 4)(*outs), 3, *c.dims(), C.byref(stats)), "f3d_validate_displacement")
        return dict(zip("ruvw", outs)), {"stats": stats}

    @staticmethod
    def verify(f3d, given, out, host):
        from test_gpu_outlier import same
        want, st = given[1], host["stats"]
        for n, e in zip("ruvw", want[:4]):
            assert same(out[n], e), f"f3d_validate_displacement {n}"
        counts = ("present", "tested", "outliers", "replaced", "undefined")
        assert {k: getattr(st, k) for k in counts} == {k: want[4][k] for k in counts}
        assert same(np.array([st.r_max], F32), np.array([want[4]["r_max"]], F32))


# geometry A first, so that the rig changes its geometry once
CASES = [ComposeFlow, InitialFlow, InvertDisplacement, CarryField, FlowStrain, WindowStrain, PrincipalStrain, PolarDecomposition,
         FromGradient, LocalCorrelation, Motion, LabelMotion, LabelContacts, LabelComponents, NearestSeed, SplitComponents, LabelShape,
         LabelOverlap, LabelField, Histogram, ValidateDisplacement]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_entry_in_a_wide_container(f3d, rigs, case):
    what = " + ".join(case.entries)
    dims = case.dims()
    hc, dc, _ = GEOMETRY[case.geometry]
    rig = rigs.get(hc, dc)
    assert_premises(rig, dims, case.geometry, what)
    given = case.given()

    dense = DenseBox(f3d, dims)
    try:
        dense_out, dense_host = case.launch(f3d, dense, given)
        f3d.sync()
        dense_boxes = {n: dense.get(p) for n, p in dense_out.items()}
        assert dense.margins_hold_the_fill(), f"{what}: written outside the box of the dense container"
    finally:
        dense.free()

    wide = WideBox(rig, dims)
    wide_out, wide_host = case.launch(f3d, wide, given)
    f3d.sync()
    boxes = {n: wide.get(p) for n, p in wide_out.items()}

    # (1) the dense container and the views of the rig give the same words: every output and every host result is looked at
    assert set(boxes) == set(dense_boxes) and set(wide_host) == set(dense_host)
    differ = []
    for n in boxes:
        bad = int((wc.words(boxes[n]) != wc.words(dense_boxes[n])).sum())
        print(f"{what}: output {n}: {bad} of {boxes[n].size} words differ from the dense container's")
        if bad:
            differ.append(f"output {n} ({bad} words)")
    differ += [f"host result {n}" for n in wide_host if raw(wide_host[n]) != raw(dense_host[n])]
    assert not differ, f"{what}: the result depends on the container's geometry: {', '.join(differ)}"
    # (2) nothing outside the box: outputs, margins, the strips behind the outputs, every input
    for n, p in wide_out.items():
        wide.views.expect(p, dense_boxes[n])
    wide.views.check(what)
    # (3) the restatement of the entry's own test, under that test's bound
    case.verify(f3d, given, boxes, wide_host)
    print(f"{what}: equal to the dense container word for word and to the restatement under its own bound; {len(boxes)} output volumes, "
          f"{len(wide_host)} host results")
