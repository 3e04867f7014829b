"""The two-class cut of the fused solver launches (csrc/f3d_pair8_plan.h: the first tiles march whole columns, only the remainder is
cut in z) on the GPU.  F3D_PAIR8_ROUND makes a round of 8 (or 16) workgroups so that tiny volumes have both classes, F3D_PAIR8_TY pins
the tile height.  Every output array of every fused entry must carry the same bits as

  * the same entry under F3D_PAIR8_PLAN=0 (the uniform plan) -- over the WHOLE container: outputs start as NaN, so a store outside the
    box or the window shows;
  * the composition of the one-sweep launches (f3d_solve_sweep, f3d_solve_sweep again on its result, f3d_phi_ksi on the first
    sweep's result), computed once per shape on the whole volume.

Each case asserts its premise through the exposed plan (both classes exist: A > 0 and T - A > 0) and its tile count.

100 x 41 x 13 at 4 rows (T = 22) cannot have both classes in rounds of 8: whole columns for 16 tiles cost 2 x 20 steps and the six
tiles left one round of 20 more (two chunks each would be two rounds of 14), 60 steps -- exactly the uniform plan's three rounds of
20, and a tie keeps the uniform plan.  The shape therefore runs twice: in rounds of 8, where the premise asserted is that tie
(A = 0, cost 60), and in rounds of 16, where both classes exist (A = 16, six tiles in two chunks of 7 planes).

xcd_remap is read once per process (F3D_XCD_REMAP), so the cases with the hardware's round robin run once more in a child.
Which one-line mutants of the decode each test catches is written down in LABBOOK.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bit_same, box_in_container

pytestmark = pytest.mark.gpu

H_SPACING = (1.3, 0.9, 2.0)
ALPHA, EPS_S, EPS_D = 7.5, 0.001, 0.002

# (W, H, D), rows per tile, workgroups per round, folds, tiles, window or None, premise: "both" classes or the "tie" described above
CASES = (
    ((70, 26, 9), 4, 8, True, 11, None, "both"),
    ((140, 30, 11), 8, 8, True, 10, None, "both"),
    ((100, 41, 13), 4, 8, False, 22, None, "tie"),
    ((100, 41, 13), 4, 16, False, 22, None, "both"),
    ((100, 61, 10), 12, 8, False, 12, None, "both"),
    ((180, 11, 8), 4, 8, False, 9, None, "one-plane chunks"),   # eight whole columns and one tile in eight chunks of one plane
    ((100, 61, 13), 12, 8, False, 12, (3, 10), "both"),
)


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


def only_the_box(got, exp, zs, dims):
    """got[z0:z1, :H, :W] carries exp's bits there and everything else of the container is still NaN"""
    W, H, _ = dims
    z0, z1 = zs
    if not bit_same(got[z0:z1, :H, :W], exp[z0:z1, :H, :W]):
        return False
    rest = np.ones(got.shape, bool)
    rest[z0:z1, :H, :W] = False
    return bool(np.isnan(got[rest]).all())


def check_premise(f3d, dims, ty, per_round, fold, tiles, window, premise):
    W, H, D = dims
    planes = D if window is None else window[1] - window[0]
    plan = f3d.pair8_plan(W, H, planes, ty, fold=fold)   # rounds from F3D_PAIR8_ROUND, as the launcher reads them
    assert plan == f3d.pair8_plan(W, H, planes, ty, per_round=per_round, fold=fold)
    assert plan.tiles == tiles, plan
    if premise == "tie":
        assert plan.A == 0 and plan.cost == 60, plan
    else:
        assert plan.A > 0 and plan.tiles - plan.A > 0, plan
        assert plan.a == 1 and plan.zc_a == planes, plan   # whole columns
    if premise == "one-plane chunks":
        assert plan.zc_b == 1 and plan.b == planes, plan


def run_case(f3d, dims, ty, per_round, fold, tiles, window, premise):
    W, H, D = dims
    cdims = ((W + 63) // 64 * 64, H + 3, D)
    rng = np.random.default_rng(1000 * W + 10 * H + D)
    mk = lambda lo, hi: box_in_container(rng, dims, cdims, lo, hi)
    arrs = [mk(0, 255), mk(0, 255), mk(-3, 3), mk(-3, 3), mk(-3, 3), mk(-0.5, 0.5), mk(-0.5, 0.5), mk(-0.5, 0.5)]
    h = H_SPACING
    hip = f3d.hip()
    tag = f"{W}x{H}x{D}, {ty} rows, rounds of {per_round}, window {window}"
    os.environ["F3D_PAIR8_TY"] = str(ty)
    os.environ["F3D_PAIR8_ROUND"] = str(per_round)
    os.environ.pop("F3D_PAIR8_PLAN", None)
    dev = Dev(f3d, cdims)
    try:
        check_premise(f3d, dims, ty, per_round, fold, tiles, window, premise)
        ptr = [dev.put(a) for a in arrs]
        # the composition of the one-sweep launches on the whole volume: weights, sweep, sweep again / the next weights
        phi, ksi = dev.out(), dev.out()
        f3d.check(hip.f3d_phi_ksi(*ptr, W, H, D, *h, EPS_S, EPS_D, phi, ksi, None))
        s1 = [dev.out() for _ in range(3)]
        f3d.check(hip.f3d_solve_sweep(*ptr, phi, ksi, W, H, D, *h, ALPHA, *s1, None))
        s2 = [dev.out() for _ in range(3)]
        f3d.check(hip.f3d_solve_sweep(*ptr[:5], *s1, phi, ksi, W, H, D, *h, ALPHA, *s2, None))
        pk = [dev.out(), dev.out()]
        f3d.check(hip.f3d_phi_ksi(*ptr[:5], *s1, W, H, D, *h, EPS_S, EPS_D, *pk, None))
        exp_two = [dev.get(p) for p in s2]
        exp_one = [dev.get(p) for p in s1 + pk]
        fd = [dev.out() for _ in range(4)]
        f3d.check(hip.f3d_frame_derivatives(ptr[0], ptr[1], W, H, D, *h, *fd, None))

        z_lo, z_hi = window or (0, D)
        slab = C.byref(f3d.Slab(0, z_lo, z_hi)) if window else None
        keeps = ((0, 0), (1, 1), (1, 0), (0, 1)) if window else ((0, 0),)
        for label, first, fdb in (("frames", ptr[:2], ""), ("derivatives", fd, "_fd")):
            entries = [("two sweeps", "f3d_solve_sweep2" + fdb, (ALPHA,), 3, (), exp_two),
                       ("sweep + phi/ksi", "f3d_solve_sweep_phi_ksi" + fdb, (ALPHA, EPS_S, EPS_D), 5, (), exp_one)]
            entries += [(f"sweep + phi/ksi, keep {k}", "f3d_solve_sweep_phi_ksi_edges" + fdb, (ALPHA, EPS_S, EPS_D), 5, k, exp_one)
                        for k in keeps if window]
            for what, entry, params, n_out, keep, exp in entries:
                got = {}
                for plan in ("1", "0"):
                    os.environ["F3D_PAIR8_PLAN"] = plan
                    outs = [dev.out() for _ in range(n_out)]
                    slab_arg = (slab if slab is not None else C.byref(f3d.Slab(0, 0, D)),) if keep else (slab,)
                    f3d.check(getattr(hip, entry)(*first, *ptr[2:], phi, ksi, W, H, D, *h, *params, *outs, *slab_arg, *keep))
                    got[plan] = [dev.get(p) for p in outs]
                for i, name in enumerate(("du", "dv", "dw", "phi", "ksi")[:n_out]):
                    where = f"{tag}, {label}, {what}: {name}"
                    assert bit_same(got["1"][i], got["0"][i]), where + " differs from the uniform plan's"
                    zs = (z_lo, z_hi)
                    if keep and i < 3:   # the sweep is kept one plane beyond the window where asked to
                        zs = (z_lo - (1 if keep[0] and z_lo > 0 else 0), z_hi + (1 if keep[1] and z_hi < D else 0))
                    assert only_the_box(got["1"][i], exp[i], zs, dims), where + " differs from the one-sweep launches'"
    finally:
        dev.close()
        for name in ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND", "F3D_PAIR8_PLAN"):
            os.environ.pop(name, None)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-ty%d-round%d%s" % (*c[0], c[1], c[2], "-window" if c[5] else ""))
def test_two_class_plans_give_the_bits_of_the_uniform_plan_and_of_the_single_sweeps(f3d, case):
    run_case(f3d, *case)


def run_all(f3d):
    for case in CASES:
        run_case(f3d, *case)


def test_the_same_with_the_hardware_round_robin():
    """xcd_remap = 0: class A chunk-major, then class B chunk-major, in workgroup order"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import importlib, sys\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import test_gpu_pair8_plan as t\n"
            "t.run_all(importlib.import_module('cuda-flow3d_amd'))\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, F3D_XCD_REMAP="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
