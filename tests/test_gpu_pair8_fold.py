"""The folded last tile column of the fused solver launches (k_pair8, csrc/f3d_solve_pair8.h): where 1 <= W mod 64 <= 32 a tile of
the last column holds two row bands side by side in the lanes.  Every case is compared bit for bit against the CPU oracle, with the
fold (the default) and with F3D_PAIR8_FOLD=0; boxes sit in the corner of NaN-poisoned containers and the outputs start as NaN, so a
store outside the box or the window shows.

Shapes.  Widths 65, 71, 95, 96 (remainder 32: lane 31 is the x face), 97 (remainder 33: must not fold -- the same bits either way),
129 and 160 (three tile columns).  Heights per forced tile height TY (F3D_PAIR8_TY = 4, 8, 12): TY (one tile row: no fold), TY + 1
(band B holds one row), 2 TY, 2 TY + 1 (odd number of tile rows: the last folded tile has an empty band B) and 3 TY + 5.  Depths 3
and 7.  The inputs are random (no symmetry in x or y); row 0 lies in band A of the first folded tile and row H-1 in band B of the
last one for every height but TY and 2 TY + 1.

Which one-line mutants of the folded body each test catches (scratch builds, run once on the MI355X, never committed) is written
down in LABBOOK.md with the measurement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu

WIDTHS = (65, 71, 95, 96, 97, 129, 160)
H_SPACING = (1.3, 0.9, 2.0)
ALPHA, EPS_S, EPS_D = 7.5, 0.001, 0.002


def heights(ty):
    return (ty, ty + 1, 2 * ty, 2 * ty + 1, 3 * ty + 5)


class Dev:
    def __init__(self, f3d, cdims):
        self.f3d, self.cdims = f3d, cdims
        self.cont = f3d.Containers(*cdims)
        self.cont.alloc(fill=0xFF)
        self.cont.set_current()

    def put(self, host_container):
        p = self.cont.new()
        self.cont.upload(p, host_container)
        return p

    def out(self):   # NaN everywhere (0xFF bytes)
        return self.cont.new()

    def get(self, p):
        self.f3d.sync()
        return self.cont.download(p, self.cdims)

    def close(self):
        self.f3d.sync()
        self.cont.free()


def solver_inputs(rng, dims, cdims):
    mk = lambda lo, hi: box_in_container(rng, dims, cdims, lo, hi)
    return [mk(0, 255), mk(0, 255), mk(-3, 3), mk(-3, 3), mk(-3, 3), mk(-0.5, 0.5), mk(-0.5, 0.5), mk(-0.5, 0.5)]


def only_the_box(got, exp, zs, dims):
    """got[z0:z1, :H, :W] equals exp's bits and everything else of the container is still NaN; zs = container planes (z0, z1), exp
    already cut to the same planes"""
    W, H, _ = dims
    z0, z1 = zs
    if not bit_same(got[z0:z1, :H, :W], exp[:, :H, :W]):
        return False
    rest = np.ones(got.shape, bool)
    rest[z0:z1, :H, :W] = False
    return bool(np.isnan(got[rest]).all())


def run_case(f3d, oracle, ty, dims):
    """every fused launch on one box, fold on and off: whole level (frames and frame derivatives), a z window of the frames builds
    in a container that starts at z_base > 0 where the depth allows, the same window of the frame-derivative builds, and the
    sweep + phi/ksi launch that keeps its edge planes"""
    W, H, D = dims
    cdims = ((W + 63) // 64 * 64, H + 3, D)
    rng = np.random.default_rng(1000 * W + 10 * H + D)
    arrs = solver_inputs(rng, dims, cdims)
    h = H_SPACING
    phi_o, ksi_o = oracle.phi_ksi(*arrs, dims, h, EPS_S, EPS_D)
    s1 = oracle.solve_sweep(*arrs, phi_o, ksi_o, dims, h, ALPHA)
    s2 = oracle.solve_sweep(*arrs[:5], *s1, phi_o, ksi_o, dims, h, ALPHA)
    phi_n, ksi_n = oracle.phi_ksi(*arrs[:5], *s1, dims, h, EPS_S, EPS_D)
    exp_two, exp_one = list(s2), list(s1) + [phi_n, ksi_n]
    z_lo, z_hi = (1, 2) if D < 7 else (3, 5)
    z_base, top = max(0, z_lo - 2), min(D, z_hi + 2)
    hip = f3d.hip()
    os.environ["F3D_PAIR8_TY"] = str(ty)
    try:
        for fold in ("1", "0"):
            os.environ["F3D_PAIR8_FOLD"] = fold
            tag = f"{W}x{H}x{D}, {ty} rows, fold {fold}"
            dev = Dev(f3d, cdims)
            try:
                ptr = [dev.put(a) for a in arrs]
                phi, ksi = dev.put(phi_o), dev.put(ksi_o)
                fd = [dev.out() for _ in range(4)]
                f3d.check(hip.f3d_frame_derivatives(ptr[0], ptr[1], W, H, D, *h, *fd, None))
                window = f3d.Slab(0, z_lo, z_hi)
                for label, first, slab, zs in (("frames", ptr[:2], None, (0, D)), ("derivatives", fd, None, (0, D)),
                                               ("derivatives, window", fd, C.byref(window), (z_lo, z_hi))):
                    fdb = "_fd" if label != "frames" else ""
                    cut = lambda a: a[zs[0]:zs[1]]
                    outs = [dev.out() for _ in range(5)]
                    f3d.check(getattr(hip, "f3d_solve_sweep2" + fdb)(*first, *ptr[2:], phi, ksi, W, H, D, *h, ALPHA, *outs[:3], slab))
                    for name, g, e in zip("uvw", outs, exp_two):
                        assert only_the_box(dev.get(g), cut(e), zs, dims), f"{tag}, {label}, two sweeps: d{name}"
                    outs = [dev.out() for _ in range(5)]
                    f3d.check(getattr(hip, "f3d_solve_sweep_phi_ksi" + fdb)(*first, *ptr[2:], phi, ksi, W, H, D, *h, ALPHA, EPS_S, EPS_D, *outs, slab))
                    for name, g, e in zip(("du", "dv", "dw", "phi", "ksi"), outs, exp_one):
                        assert only_the_box(dev.get(g), cut(e), zs, dims), f"{tag}, {label}, sweep + phi/ksi: {name}"
            finally:
                dev.close()
            # the frames builds on a window of a container whose plane 0 is plane z_base of the volume
            sub = lambda a: np.ascontiguousarray(a[z_base:top])
            zs = (z_lo - z_base, z_hi - z_base)
            dev = Dev(f3d, (cdims[0], cdims[1], top - z_base))
            try:
                ptr = [dev.put(sub(a)) for a in arrs] + [dev.put(sub(phi_o)), dev.put(sub(ksi_o))]
                slab = f3d.Slab(z_base, z_lo, z_hi)
                outs = [dev.out() for _ in range(5)]
                f3d.check(hip.f3d_solve_sweep2(*ptr, W, H, D, *h, ALPHA, *outs[:3], C.byref(slab)))
                for name, g, e in zip("uvw", outs, exp_two):
                    assert only_the_box(dev.get(g), e[z_lo:z_hi], zs, dims), f"{tag}, window, two sweeps: d{name}"
                for keep in ((0, 0), (1, 1), (1, 0), (0, 1)):
                    outs = [dev.out() for _ in range(5)]
                    f3d.check(hip.f3d_solve_sweep_phi_ksi_edges(*ptr, W, H, D, *h, ALPHA, EPS_S, EPS_D, *outs, C.byref(slab), *keep))
                    s_lo = z_lo - (1 if keep[0] and z_lo > 0 else 0)
                    s_hi = z_hi + (1 if keep[1] and z_hi < D else 0)
                    for name, g, e in zip(("du", "dv", "dw"), outs, exp_one):
                        assert only_the_box(dev.get(g), e[s_lo:s_hi], (s_lo - z_base, s_hi - z_base), dims), f"{tag}, window, keep {keep}: {name}"
                    for name, g, e in zip(("phi", "ksi"), outs[3:], exp_one[3:]):
                        assert only_the_box(dev.get(g), e[z_lo:z_hi], zs, dims), f"{tag}, window, keep {keep}: {name}"
            finally:
                dev.close()
    finally:
        os.environ.pop("F3D_PAIR8_TY", None)
        os.environ.pop("F3D_PAIR8_FOLD", None)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("ty", (4, 8, 12))
def test_folded_tiles_equal_the_oracle(f3d, oracle, ty, width):
    for height in heights(ty):
        for depth in (3, 7):
            run_case(f3d, oracle, ty, (width, height, depth))


CHUNKED_WIDTHS = (65, 96, 129)


def run_chunked(f3d, oracle):
    for ty in (4, 8, 12):
        for width in CHUNKED_WIDTHS:
            for height in (ty + 1, 2 * ty + 1, 3 * ty + 5):
                for depth in (3, 7):
                    run_case(f3d, oracle, ty, (width, height, depth))


@pytest.mark.parametrize("zchunk", ("1", "2"))
def test_folded_tiles_in_chunks_of_one_and_two_planes(zchunk):
    """Chunk prologues and the top chunk's extra step on folded tiles.  F3D_ZCHUNK is read once per process, so the pinned chunks run
    in a child: the same cases as above on three widths and the three heights with a second band."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import importlib, sys\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import test_gpu_pair8_fold as t\n"
            "from oracle import oracle as orc\n"
            "orc.lib()\n"
            "t.run_chunked(importlib.import_module('cuda-flow3d_amd'), orc)\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, F3D_ZCHUNK=zchunk), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])


def test_a_whole_pyramid_is_the_same_with_and_without_the_fold(f3d, monkeypatch):
    """A default solve of a 70 x 70 x 70 pair: the levels from 65 voxels up fold their second tile column (remainders 6 and 2)."""
    f0, f1 = f3d.synth_pair(70, 70, 70)
    flows = []
    for fold in ("1", "0"):
        monkeypatch.setenv("F3D_PAIR8_FOLD", fold)
        flow = f3d.OpticalFlow()
        flow.initialize(70, 70, 70)
        try:
            flows.append(flow.compute(f0, f1, silent=True))
        finally:
            flow.destroy()
    for name, a, b in zip("uvw", *flows):
        assert np.isfinite(a).all() and bit_same(a, b), f"flow component {name} differs between the folded and the unfolded tiling"
