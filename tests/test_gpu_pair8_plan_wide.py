"""The wide plan of the fused solver launches (csrc/f3d_pair8_plan.h: up to three classes of tiles, also where one round covers the
level) on the GPU.  F3D_PAIR8_ROUND makes a round of 8 or 16 workgroups so that tiny volumes have every class, F3D_PAIR8_TY pins the tile
height.  Every output array of every fused entry under the default plan must carry the same bits as

  * the same entry under F3D_PAIR8_PLAN=1 (the two-class plan) and under F3D_PAIR8_PLAN=0 (the uniform plan) -- over the WHOLE
    container: outputs start as NaN, so a store outside the box or the window, or a plane never stored, shows;
  * the composition of the one-sweep launches, computed once per shape on the whole volume.

Each case asserts its premise through the exposed plan of the launcher (f3d.pair8_plan_wide): its classes, its cost and the cost
of the two-class plan it beats.

130 x 37 x 26 at 4 rows in rounds of 16 has three classes and folds, but its last class is not a folded tile: 37 rows are TEN tile
rows, so the 25 tiles end with the two regular tiles of row 9 and the folded tiles are numbers 2, 7, 12, 17 and 22.  No round size
changes which tile is last; the case stays, asserting the plan it gets (16 whole columns, 8 tiles x 2 chunks, tile 24 in 13 chunks of 2
planes), and 130 x 17 x 22 in rounds of 8 -- five tile rows, 13 tiles, the last one the folded tile of row 4 whose second band is
empty -- is the shape where a folded tile is alone in the last class.

xcd_remap is read once per process (F3D_XCD_REMAP), so the cases with the hardware's round robin run once more in a child."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bit_same, box_in_container
from test_gpu_pair8_plan import ALPHA, EPS_D, EPS_S, H_SPACING, Dev, only_the_box

pytestmark = pytest.mark.gpu

# (W, H, D), rows per tile, workgroups per round, folds, window or None, classes of the plan, its cost, the two-class plan's cost,
# number of the folded tile that is alone in the last class or None
CASES = (
    ((170, 12, 20), 4, 16, False, None, ((8, 2, 10), (1, 10, 2)), 26, 27, None),          # 9 tiles: one round covers the level
    ((100, 25, 38), 4, 8, False, None, ((8, 1, 38), (4, 2, 19), (2, 4, 10)), 88, 90, None),
    ((130, 37, 26), 4, 16, True, None, ((16, 1, 26), (8, 2, 13), (1, 13, 2)), 62, 65, None),
    ((130, 17, 22), 4, 8, True, None, ((8, 1, 22), (4, 2, 11), (1, 8, 3)), 57, 58, 12),
    ((130, 52, 27), 12, 8, True, (3, 25), ((8, 1, 22), (4, 2, 11), (1, 8, 3)), 57, 58, 12),
)


def check_premise(f3d, dims, ty, per_round, fold, window, classes, cost, parent_cost, folded_last):
    W, H, D = dims
    z_lo, z_hi = window or (0, D)
    plan = f3d.pair8_plan_wide(W, H, z_hi - z_lo, ty, fold=fold)   # rounds and switch from the environment, as the launcher reads them
    assert plan == f3d.pair8_plan_wide(W, H, z_hi - z_lo, ty, per_round=per_round, fold=fold)
    assert plan.tiles == sum(c[0] for c in classes), plan
    assert plan.classes == classes and plan.cost == cost, plan
    assert f3d.pair8_plan(W, H, z_hi - z_lo, ty, fold=fold).cost == parent_cost
    if fold:
        wg = f3d.pair8_decode_wide(W, H, ty, fold, plan, 0, z_lo, z_hi)
        last = wg[wg[:, 0] >= plan.tiles - classes[-1][0]]
        assert len(last) == classes[-1][0] * classes[-1][1]
        if folded_last is None:
            assert (last[:, 3] == 0).all(), last
        else:
            assert classes[-1][0] == 1 and (last[:, 0] == folded_last).all() and (last[:, 3] == 1).all(), last
        assert (wg[:, 3] == 1).any()


def run_case(f3d, dims, ty, per_round, fold, window, *premise):
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
        check_premise(f3d, dims, ty, per_round, fold, window, *premise)
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
                for plan in (None, "1", "0"):   # None: the default, the wide plan
                    if plan is None:
                        os.environ.pop("F3D_PAIR8_PLAN", None)
                    else:
                        os.environ["F3D_PAIR8_PLAN"] = plan
                    outs = [dev.out() for _ in range(n_out)]
                    slab_arg = (slab if slab is not None else C.byref(f3d.Slab(0, 0, D)),) if keep else (slab,)
                    f3d.check(getattr(hip, entry)(*first, *ptr[2:], phi, ksi, W, H, D, *h, *params, *outs, *slab_arg, *keep))
                    got[plan] = [dev.get(p) for p in outs]
                os.environ.pop("F3D_PAIR8_PLAN", None)
                for i, name in enumerate(("du", "dv", "dw", "phi", "ksi")[:n_out]):
                    where = f"{tag}, {label}, {what}: {name}"
                    assert bit_same(got[None][i], got["1"][i]), where + " differs from the two-class plan's"
                    assert bit_same(got[None][i], got["0"][i]), where + " differs from the uniform plan's"
                    zs = (z_lo, z_hi)
                    if keep and i < 3:   # the sweep is kept one plane beyond the window where asked to
                        zs = (z_lo - (1 if keep[0] and z_lo > 0 else 0), z_hi + (1 if keep[1] and z_hi < D else 0))
                    assert only_the_box(got[None][i], exp[i], zs, dims), where + " differs from the one-sweep launches'"
    finally:
        dev.close()
        for name in ("F3D_PAIR8_TY", "F3D_PAIR8_ROUND", "F3D_PAIR8_PLAN"):
            os.environ.pop(name, None)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-ty%d-round%d%s" % (*c[0], c[1], c[2], "-window" if c[4] else ""))
def test_wide_plans_give_the_bits_of_the_other_plans_and_of_the_single_sweeps(f3d, case):
    run_case(f3d, *case)


def run_all(f3d):
    for case in CASES:
        run_case(f3d, *case)


def test_the_same_with_the_hardware_round_robin():
    """xcd_remap = 0: the classes one after the other, each chunk-major, in workgroup order"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import importlib, sys\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import test_gpu_pair8_plan_wide as t\n"
            "t.run_all(importlib.import_module('cuda-flow3d_amd'))\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, F3D_XCD_REMAP="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
