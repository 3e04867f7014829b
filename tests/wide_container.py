"""A container whose planes are hundreds of MiB, for tests/test_gpu_wide_container_offsets.py (and its child interpreter,
tests/wide_container_worker.py) and tests/test_gpu_wide_container_analysis.py.

An address depends on the container's geometry (height, pitch), not on the box: a 70 x 20 x 19 box in the corner of a container whose
planes are 256 MiB forms the byte offsets a huge volume forms.  ONE device allocation of 8192 x 8192 x 20 floats (pitch 32 768 bytes,
5 GiB) is filled with 0xFF once; every "container" of a test is a VIEW into it -- the base pointer plus k * strip rows, strip >= H + 2
-- under the one geometry (8192, 8192, 20, pitch).  Kernels touch rows < H of planes < D of a view only, so views do not overlap.

Host memory: nothing is page-locked, and nothing larger than a box with its margin (a few hundred KB) is ever built or freed: boxes
and margins are downloaded, never a container."""
import ctypes as C

import numpy as np

WC = 8192
PITCH = WC * 4
FILL = 0xFFFFFFFF
MX, MY = 3, 2          # the margin looked at around a box: columns, rows (and one plane either side of the planes written)
HOST_BLOCK_LIMIT = 660_000   # bytes: the largest block the suite builds and frees elsewhere in the process


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bit_same(a, b):
    return a.shape == b.shape and bool(np.all(words(a) == words(b)))


class Wide:
    def __init__(self, f3d, hc=8192, dc=20):
        self.f3d, self.hip = f3d, f3d.hip()
        self.hc, self.dc = hc, dc
        self.cont = f3d.Containers(WC, hc, dc)
        self.base = self.cont.alloc(fill=0xFF)
        assert self.cont.pitch == PITCH, self.cont.pitch
        self.rows = hc * dc
        self.plane_bytes = PITCH * hc
        self.strip = self.count = 0
        self.cont.set_current()

    def geometry(self, hc):
        """another container height over the same allocation, which still covers it: planes of hc rows, not more rows in all"""
        assert hc * self.dc <= self.rows
        self.hc = self.cont.height = hc
        self.plane_bytes = PITCH * hc
        self.cont.set_current()

    def close(self):
        self.f3d.sync()
        self.cont.free()

    def begin(self, dims):
        """a new case on a W x H x . box: every strip is free again and holds the fill (columns < W + MX of every row)"""
        W, H, _ = dims
        self.dims = dims
        self.strip, self.count = H + MY, 0
        self.cont.set_current()
        self.f3d.check(self.hip.f3d_memset2d(self.base, PITCH, 0xFF, (W + MX) * 4, self.rows))

    def view(self):
        k = self.count
        assert k * self.strip + self.dims[1] <= self.hc, "the views leave the allocation"
        self.count += 1
        return self.base + k * self.strip * PITCH

    def upload(self, ptr, vol, plane0=0):
        vol = np.ascontiguousarray(vol, np.float32)
        assert vol.nbytes <= HOST_BLOCK_LIMIT
        d, h, w = vol.shape
        assert plane0 + d <= self.dc and h <= self.strip
        self.f3d.check(self.hip.f3d_copy3d_h2d(ptr, PITCH, self.hc, plane0, vol.ctypes.data_as(C.POINTER(C.c_float)), w, h, d))

    def put(self, vol, plane0=0):
        p = self.view()
        self.upload(p, vol, plane0)
        return p

    def download(self, ptr, w, h, planes):
        """container planes [planes[0], planes[1]) of a view, rows < h, columns < w"""
        p0, p1 = planes
        assert 0 <= p0 < p1 <= self.dc and h <= self.strip
        out = np.empty((p1 - p0, h, w), np.float32)
        assert out.nbytes <= HOST_BLOCK_LIMIT
        self.f3d.sync()
        self.f3d.check(self.hip.f3d_copy3d_d2h(out.ctypes.data_as(C.POINTER(C.c_float)), w, h, p1 - p0, ptr, PITCH, self.hc, p0))
        return out

    def out(self):
        """an output view and the untouched strip behind it"""
        return self.view(), self.view()

    def written(self, pair, planes):
        """Box and margin of an output view: (the box over container planes `planes`, True if the margin -- MX columns, MY rows, the
        plane on either side -- and the strip behind the view still hold the fill)"""
        W, H, _ = self.dims
        ptr, guard = pair
        p0, p1 = planes
        q0, q1 = max(p0 - 1, 0), min(p1 + 1, self.dc)
        got = self.download(ptr, W + MX, H + MY, (q0, q1))
        box = got[p0 - q0:p1 - q0, :H, :W].copy()
        rest = np.ones(got.shape, bool)
        rest[p0 - q0:p1 - q0, :H, :W] = False
        clean = bool((words(got)[rest] == FILL).all())
        behind = self.download(guard, W + MX, H + MY, (q0, q1))
        return box, clean and bool((words(behind) == FILL).all())

    def unchanged(self, ptr, vol, plane0=0):
        d, h, w = vol.shape
        return bit_same(self.download(ptr, w, h, (plane0, plane0 + d)), vol)


class Rigs:
    """one allocation at a time, shared by the tests of a module: rigs.get(8192, 20) is the 256 MiB geometry (5 GiB), get(4096, 40) the
    same 5 GiB as planes of 128 MiB, get(13654, 9) the y march's (3.8 GiB)"""

    def __init__(self, f3d):
        self.f3d, self.kind, self.rig = f3d, None, None

    def get(self, hc, dc):
        if self.kind != (hc, dc):
            self.close()
            self.rig, self.kind = Wide(self.f3d, hc, dc), (hc, dc)
        return self.rig

    def close(self):
        if self.rig is not None:
            self.rig.close()
        self.rig = self.kind = None


# ---- the solver family ------------------------------------------------------------------------------------------------------------

H3 = (1.3, 0.9, 2.0)
ALPHA = 7.5
EPS = (0.001, 0.001)

# name -> (kernel family, halo planes read on either side of a chunk)
SOLVER_ENTRIES = {
    "f3d_phi_ksi": ("one", 1),
    "f3d_phi_ksi_zones": ("one", 1),
    "f3d_solve_sweep": ("one", 1),
    "f3d_solve_sweep_add": ("one", 1),
    "f3d_solve_sweep2": ("pair", 2),
    "f3d_solve_sweep2_fd": ("pair", 2),
    "f3d_solve_sweep_phi_ksi": ("pair", 2),
    "f3d_solve_sweep_phi_ksi_edges": ("pair", 2),
    "f3d_solve_sweep_phi_ksi_fd": ("pair", 2),
    "f3d_solve_sweep_phi_ksi_edges_fd": ("pair", 2),
    "f3d_solve_phi_ksi_sweep_fd": ("pair", 2),
    "f3d_solve_sweep2_add_fd": ("pair", 2),
    "f3d_solve_sweep3": ("tri", 3),
    "f3d_solve_sweep2_phi_ksi": ("tri", 3),
}


def solver_hosts(dims, seed):
    """the eight inputs of the solver on a dense W x H x D box (the oracle's container is the box itself)"""
    W, H, D = dims
    rng = np.random.default_rng(seed)
    mk = lambda lo, hi: rng.uniform(lo, hi, size=(D, H, W)).astype(np.float32)
    return [mk(0, 255), mk(0, 255), mk(-3, 3), mk(-3, 3), mk(-3, 3), mk(-0.5, 0.5), mk(-0.5, 0.5), mk(-0.5, 0.5)]


def frame_derivatives_ref(f0, f1, h):
    """fx, fy, fz, ft as k_frame_derivatives forms them: the numerator left to right in binary32, one division by 4 h"""
    out = []
    for axis, step in ((2, h[0]), (1, h[1]), (0, h[2])):
        n = f0.shape[axis]
        up = np.minimum(np.arange(n) + 1, n - 1)
        up[n - 1] = n - 2
        dn = np.abs(np.arange(n) - 1)
        a, b = (np.take(f0, up, axis), np.take(f0, dn, axis)), (np.take(f1, up, axis), np.take(f1, dn, axis))
        num = ((a[0] - a[1]) + b[0]) - b[1]
        out.append((num / (np.float32(4.0) * np.float32(step))).astype(np.float32))
    out.append(f1 - f0)
    assert all(o.dtype == np.float32 for o in out)
    return out


def solver_expectations(oracle, hosts, dims):
    """What every entry must produce, from the oracle's one-stage functions on the dense box."""
    a5, h = hosts[:5], H3
    phi, ksi = oracle.phi_ksi(*hosts, dims, h, *EPS)
    s1 = oracle.solve_sweep(*hosts, phi, ksi, dims, h, ALPHA)
    s2 = oracle.solve_sweep(*a5, *s1, phi, ksi, dims, h, ALPHA)
    s3 = oracle.solve_sweep(*a5, *s2, phi, ksi, dims, h, ALPHA)
    pk1 = oracle.phi_ksi(*a5, *s1, dims, h, *EPS)
    pk2 = oracle.phi_ksi(*a5, *s2, dims, h, *EPS)

    def added(inc):
        sums = [a.copy() for a in hosts[2:5]]
        for s, i in zip(sums, inc):
            oracle.add(s, i, dims)
        return sums
    return {"weights": [phi, ksi], "s1": list(s1), "s2": list(s2), "s3": list(s3), "s1+pk": list(s1) + list(pk1),
            "s2+pk": list(s2) + list(pk2), "pk+s1": [phi, ksi] + list(s1), "u+s1": added(s1), "u+s2": added(s2),
            "fd": frame_derivatives_ref(hosts[0], hosts[1], h)}


class SolverCase:
    """The solver's inputs of one box in views of a Wide container.  `window` = (z_base, z_lo, z_hi) or None: the container holds the
    global planes z_base .. z_base + 18 of a level of dims[2] planes."""

    def __init__(self, rig, hosts, weights, dims, window):
        self.rig, self.f3d, self.hip = rig, rig.f3d, rig.hip
        self.dims, self.window = dims, window
        W, H, D = dims
        self.z_base, self.z_lo, self.z_hi = window or (0, 0, D)
        self.held = (self.z_base, min(D, self.z_base + rig.dc - 1))      # global planes in the container
        rig.begin(dims)
        self.hosts = [np.ascontiguousarray(a[self.held[0]:self.held[1]]) for a in list(hosts) + list(weights)]
        self.ptr = [rig.put(a) for a in self.hosts]
        self.slab = C.byref(self.f3d.Slab(self.z_base, self.z_lo, self.z_hi)) if window else None
        self.fd = None

    def planes(self, zs):
        return zs[0] - self.z_base, zs[1] - self.z_base

    def launch(self, name, keep=None, zones=None):
        """-> (names of the outputs' expectations, output views, global planes each output is written on)"""
        f3d, hip, p = self.f3d, self.hip, self.ptr
        W, H, D = self.dims
        dims_h = (W, H, D, *H3)
        zs = (self.z_lo, self.z_hi)
        fd = self.fd
        new = lambda n: [self.rig.out() for _ in range(n)]
        ptrs = lambda outs: [o[0] for o in outs]
        if name == "f3d_frame_derivatives":
            outs, key = new(4), "fd"
            f3d.check(hip.f3d_frame_derivatives(p[0], p[1], *dims_h, *ptrs(outs), self.slab))
        elif name == "f3d_phi_ksi":
            outs, key = new(2), "weights"
            f3d.check(hip.f3d_phi_ksi(*p[:8], *dims_h, *EPS, *ptrs(outs), self.slab))
        elif name == "f3d_phi_ksi_zones":
            outs, key = new(2), "weights"
            za, zb = (C.byref(f3d.Slab(self.z_base, *z)) for z in zones)
            f3d.check(hip.f3d_phi_ksi_zones(*p[:8], *dims_h, *EPS, *ptrs(outs), za, zb))
        elif name in ("f3d_solve_sweep", "f3d_solve_sweep_add", "f3d_solve_sweep2", "f3d_solve_sweep3"):
            outs = new(3)
            key = {"f3d_solve_sweep": "s1", "f3d_solve_sweep_add": "u+s1", "f3d_solve_sweep2": "s2", "f3d_solve_sweep3": "s3"}[name]
            fn = f3d.solve_sweep_add_entry() if name == "f3d_solve_sweep_add" else getattr(hip, name)
            f3d.check(fn(*p[:10], *dims_h, ALPHA, *ptrs(outs), self.slab))
        elif name == "f3d_solve_sweep2_fd":
            outs, key = new(3), "s2"
            f3d.check(hip.f3d_solve_sweep2_fd(*fd, *p[2:10], *dims_h, ALPHA, *ptrs(outs), self.slab))
        elif name in ("f3d_solve_sweep_phi_ksi", "f3d_solve_sweep2_phi_ksi"):
            outs, key = new(5), "s1+pk" if name == "f3d_solve_sweep_phi_ksi" else "s2+pk"
            f3d.check(getattr(hip, name)(*p[:10], *dims_h, ALPHA, *EPS, *ptrs(outs), self.slab))
        elif name == "f3d_solve_sweep_phi_ksi_fd":
            outs, key = new(5), "s1+pk"
            f3d.check(hip.f3d_solve_sweep_phi_ksi_fd(*fd, *p[2:10], *dims_h, ALPHA, *EPS, *ptrs(outs), self.slab))
        elif name in ("f3d_solve_sweep_phi_ksi_edges", "f3d_solve_sweep_phi_ksi_edges_fd"):
            outs, key = new(5), "s1+pk"
            first = fd if name.endswith("_fd") else p[:2]
            slab = self.slab if self.slab is not None else C.byref(f3d.Slab(0, 0, D))
            f3d.check(getattr(hip, name)(*first, *p[2:10], *dims_h, ALPHA, *EPS, *ptrs(outs), slab, *keep))
        elif name == "f3d_solve_phi_ksi_sweep_fd":
            outs, key = new(5), "pk+s1"
            f3d.check(f3d.solve_phi_ksi_sweep_fd_entry()(*fd, *p[2:8], *dims_h, ALPHA, *EPS, *ptrs(outs), None))
        elif name == "f3d_solve_sweep2_add_fd":
            outs, key = new(3), "u+s2"
            f3d.check(f3d.solve_sweep2_add_fd_entry()(*fd, *p[2:10], *dims_h, ALPHA, *ptrs(outs), None))
        else:
            raise KeyError(name)
        spans = [zs] * len(outs)
        if keep:   # the sweep is kept one plane beyond the window where asked to
            kept = (zs[0] - (1 if keep[0] and zs[0] > 0 else 0), zs[1] + (1 if keep[1] and zs[1] < D else 0))
            spans = [kept] * 3 + [zs] * 2
        return key, outs, spans

    def run(self, name, keep=None, zones=None):
        """One launch.  -> {expectation key, global planes, boxes}: the boxes the launch wrote, after the three checks every launch
        gets -- margin and the strip behind every output still the fill, every input unchanged."""
        key, outs, spans = self.launch(name, keep, zones)
        boxes = []
        for i, (o, zs) in enumerate(zip(outs, spans)):
            if zones:   # two windows: whatever lies between them stays the fill
                (a0, a1), (b0, b1) = sorted(zones)
                box, clean = self.rig.written(o, self.planes((a0, b1)))
                gap = box[a1 - a0:b0 - a0]
                clean = clean and bool((words(gap) == FILL).all())
                box = np.concatenate([box[:a1 - a0], box[b0 - a0:]])
            else:
                box, clean = self.rig.written(o, self.planes(zs))
            assert clean, f"{name}: output {i} wrote outside planes {zs} of the box, or into the next strip"
            boxes.append(box)
        for i, (ptr, host) in enumerate(zip(self.ptr, self.hosts)):
            assert self.rig.unchanged(ptr, host), f"{name}: input {i} was written"
        if self.fd is not None:
            for i, (ptr, host) in enumerate(zip(self.fd, self.fd_hosts)):
                assert self.rig.unchanged(ptr, host, self.fd_span[0] - self.z_base), f"{name}: frame derivative {i} was written"
        return {"key": key, "spans": spans, "zones": zones, "boxes": boxes}

    def make_frame_derivatives(self):
        """fx, fy, fz, ft of the planes the container holds, by the kernel (whole container window: its halo must be inside)"""
        W, H, D = self.dims
        lo = self.held[0] + (1 if self.held[0] > 0 else 0)
        hi = self.held[1] - (1 if self.held[1] < D else 0)
        slab, window = self.slab, (self.z_lo, self.z_hi)
        self.slab = C.byref(self.f3d.Slab(self.z_base, lo, hi)) if self.window else None
        self.z_lo, self.z_hi = lo, hi
        res = self.run("f3d_frame_derivatives")
        self.slab, (self.z_lo, self.z_hi) = slab, window
        # the views the derivative entries read: planes lo .. hi hold values, the rest the fill (never read: reach 2 of [z_lo, z_hi))
        self.fd_span = (lo, hi)
        self.fd_hosts = res["boxes"]
        self.fd = [self.rig.put(b, plane0=lo - self.z_base) for b in res["boxes"]]
        return res


def expected_boxes(expect, res, dims):
    """the oracle's values over the planes a launch wrote, in the order of its outputs"""
    out = []
    for e, zs in zip(expect[res["key"]], res["spans"]):
        if res["zones"]:
            (a0, a1), (b0, b1) = sorted(res["zones"])
            out.append(np.concatenate([e[a0:a1], e[b0:b1]]))
        else:
            out.append(e[zs[0]:zs[1]])
    return out


def chunk_reach(z0, z1, reach, depth):
    """first and last plane a chunk [z0, z1) loads: `reach` planes either side, mirrored back into the level at its faces"""
    return max(z0 - reach, 0), min(z1 - 1 + reach, depth - 1)


def largest_offset(chunks, reach, depth, plane_bytes):
    """(largest byte offset of a plane from its chunk's first plane, longest chunk) over chunks [(z0, z1), ...]"""
    spans = [chunk_reach(z0, z1, reach, depth) for z0, z1 in chunks]
    return max(hi - lo for lo, hi in spans) * plane_bytes, max(z1 - z0 for z0, z1 in chunks)


def uniform_chunks(z_lo, z_hi, zchunk):
    return [(z, min(z + zchunk, z_hi)) for z in range(z_lo, z_hi, zchunk)]


def assert_premises(chunks, reach, depth, plane_bytes, zc_limit, what):
    """(a) the window is longer than a chunk may be, (b) a chunk forms a byte offset of 2^31 or more, (c) no chunk passes the limit"""
    planes = max(z1 for _, z1 in chunks) - min(z0 for z0, _ in chunks)
    offset, longest = largest_offset(chunks, reach, depth, plane_bytes)
    assert planes > zc_limit, f"{what}: (a) {planes} planes fit one chunk of {zc_limit}"
    assert offset >= 1 << 31, f"{what}: (b) the largest offset formed is {offset}"
    assert longest <= zc_limit and offset + plane_bytes <= 1 << 32, f"{what}: (c) a chunk of {longest} planes, limit {zc_limit}"
    return offset


# ---- the launches of the child interpreter (F3D_ZCHUNK=7, F3D_PAIR8=0) ----
WINDOW = (9, 13, 26)      # container plane 0 holds global plane 9 of 28; planes [13, 26) are produced: 13 > 7 planes
# tag, dims, window, the two windows of f3d_phi_ksi_zones (eight or nine planes each, off the level's faces; the plane between them stays untouched)
CHILD_CASES = [("whole", (70, 20, 19), None, ((1, 9), (10, 19))),
               ("window", (70, 20, 28), WINDOW, ((10, 18), (19, 27)))]
# entry, F3D_TRI_TY (0: not a three-stage launch); with F3D_PAIR8=0 f3d_solve_sweep2 is k_sweep7
CHILD_LAUNCHES = [("f3d_phi_ksi", 0), ("f3d_phi_ksi_zones", 0), ("f3d_solve_sweep", 0), ("f3d_solve_sweep_add", 0),
                  ("f3d_solve_sweep2", 0), ("f3d_solve_sweep3", 4), ("f3d_solve_sweep3", 7), ("f3d_solve_sweep2_phi_ksi", 4),
                  ("f3d_solve_sweep2_phi_ksi", 7)]
CHILD_KEYS = {"f3d_phi_ksi": "weights", "f3d_phi_ksi_zones": "weights", "f3d_solve_sweep": "s1", "f3d_solve_sweep_add": "u+s1",
              "f3d_solve_sweep2": "s2", "f3d_solve_sweep3": "s3", "f3d_solve_sweep2_phi_ksi": "s2+pk"}
CHILD_KERNELS = {"f3d_phi_ksi": "k_phiksi6", "f3d_phi_ksi_zones": "k_phiksi6", "f3d_solve_sweep": "k_sweep6",
                 "f3d_solve_sweep_add": "k_last_sweep_flow", "f3d_solve_sweep2": "k_sweep7", "f3d_solve_sweep3": "k_tri<SSS>",
                 "f3d_solve_sweep2_phi_ksi": "k_tri<SSP>"}


# ---- streaming passes and plane movers: every view has an image of what it must hold -------------------------------------------------

def dev_array(ptrs):
    return (C.c_uint64 * len(ptrs))(*ptrs)


class Views:
    """Views of a Wide container for boxes of up to W x H, each with a host image of its first `planes` planes, rows < H + MY, columns
    < W + MX: what was uploaded, what a launch is expected to have written since, and the fill everywhere else.  check() compares every
    view with its image, word for word: outputs, the margin around them, the untouched strips behind them and every input at once."""

    def __init__(self, rig, dims, planes=None):
        self.rig = rig
        rig.begin(dims)
        self.w, self.h = dims[0] + MX, dims[1] + MY
        self.planes = planes or rig.dc
        assert self.planes * self.h * self.w * 4 <= HOST_BLOCK_LIMIT
        self.image, self.by_value = {}, set()

    def new(self, vol=None, plane0=0, guard=False, x0=0):
        """a view, optionally holding `vol` from container plane `plane0` and column `x0` on; use p + 4 * x0 to address that box"""
        p = self.rig.view()
        self.image[p] = np.full((self.planes, self.h, self.w), FILL, np.uint32).view(np.float32)
        if vol is not None:
            self.rig.upload(p + 4 * x0, vol, plane0)
            self.expect(p, vol, plane0, x0=x0)
        if guard:   # the strip behind an output stays untouched
            self.new()
        return p

    def expect(self, p, box, plane0=0, y0=0, x0=0):
        d, h, w = box.shape
        self.image[p][plane0:plane0 + d, y0:y0 + h, x0:x0 + w] = box

    def check(self, what):
        for k, (p, want) in enumerate(self.image.items()):
            got = self.rig.download(p, self.w, self.h, (0, self.planes))
            diff = words(got) != words(want)
            if p in self.by_value:   # medians: -0 and +0 are the same value
                diff &= ~(got == want)
            if diff.any():
                z, y, x = (int(i) for i in np.argwhere(diff)[0])
                raise AssertionError(f"{what}: view {k}: {int(diff.sum())} words are not what they must be; first at plane {z} row {y} "
                                     f"column {x}: {got[z, y, x]!r}, expected {want[z, y, x]!r}")
