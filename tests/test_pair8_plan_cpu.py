"""The cut of a fused solver launch into workgroups (csrc/f3d_pair8_plan.h), without a GPU: the plan through f3d_pair8_plan and the
kernel's own decode of a workgroup number -- one __host__ __device__ function, compiled into the host library as well -- through
f3d_pair8_decode.

The round model is restated here as it stood before the two-class plan (one chunk length for every tile), so "never dearer than the
uniform plan" and "F3D_PAIR8_PLAN=0 is the uniform plan" are checked against this file's arithmetic, not against the library's."""
import importlib

import numpy as np
import pytest

f3d = importlib.import_module("cuda-flow3d_amd")

EXTRA = 7   # steps a chunk costs beside its planes (F3D_PAIR8_CHUNK_STEPS is not set in the suite)

WIDTHS = (64, 65, 96, 130, 200, 439, 600)
ROWS = (1, 13, 61, 200, 520)
PLANES = (1, 2, 3, 7, 13, 103, 439, 520)


def tiles_of(width, rows, ty, fold):
    ntx, nty = -(-width // 64), -(-rows // ty)
    return (ntx - 1) * nty + (nty + 1) // 2 if fold else ntx * nty


def may_fold(width, rows, ty):
    return 1 <= width % 64 <= 32 and width > 64 and rows > ty


def uniform_plan(tiles, planes, zc_limit, per_round):
    """(zchunk, cost, workgroups) of the plan with one chunk length: the first cheapest of 1 .. planes chunks"""
    best = None
    for nzc in range(1, planes + 1):
        zc = -(-planes // nzc)
        if zc > zc_limit:
            continue
        wgs = tiles * -(-planes // zc)
        cost = -(-wgs // per_round) * (zc + EXTRA)
        if best is None or cost < best[1]:
            best = (zc, cost, wgs)
    return best


def tile_places(width, rows, ty, fold):
    """tile number -> (tile column, tile row, folded) in the numbering of the fused launches"""
    ntx, nty = -(-width // 64), -(-rows // ty)
    if not fold:
        return [(t % ntx, t // ntx, 0) for t in range(ntx * nty)]
    out = []
    for pair in range((nty + 1) // 2):
        out += [(x, 2 * pair, 0) for x in range(ntx - 1)] + [(ntx - 1, 2 * pair, 1)]
        if 2 * pair + 1 < nty:
            out += [(x, 2 * pair + 1, 0) for x in range(ntx - 1)]
    return out


def check_decode(width, rows, planes, ty, fold, plan, z_lo, tag):
    places = np.array(tile_places(width, rows, ty, fold), np.int32)
    assert len(places) == plan.tiles, tag
    for remap in (0, 1):
        wg = f3d.pair8_decode(width, rows, ty, fold, plan, remap, z_lo, z_lo + planes)
        valid = wg[:, 0] >= 0
        assert (wg[~valid] == -1).all(), tag
        # no workgroup without planes; only an XCD's run is padded, by less than eight numbers per class
        assert int(valid.sum()) == plan.wgs and len(wg) - plan.wgs <= (14 if remap else 0), (tag, remap, len(wg))
        w = wg[valid]
        assert (w[:, 5] > w[:, 4]).all() and (w[:, 4] >= z_lo).all() and (w[:, 5] <= z_lo + planes).all(), (tag, remap)
        in_a = w[:, 0] < plan.A
        assert ((w[:, 5] - w[:, 4])[in_a] <= plan.zc_a).all() and ((w[:, 5] - w[:, 4])[~in_a] <= plan.zc_b).all(), (tag, remap)
        assert (w[:, 1:4] == places[w[:, 0]]).all(), (tag, remap)
        # every (tile, plane) exactly once
        cover = np.zeros((plan.tiles, planes + 1), np.int64)
        np.add.at(cover, (w[:, 0], w[:, 4] - z_lo), 1)
        np.add.at(cover, (w[:, 0], w[:, 5] - z_lo), -1)
        assert (np.cumsum(cover, axis=1)[:, :planes] == 1).all(), (tag, remap)
        if not remap:   # class A chunk-major, then class B chunk-major
            n_a = plan.A * plan.a
            assert (w[:n_a, 0] == np.tile(np.arange(plan.A), plan.a)).all(), tag
            assert (w[n_a:, 0] == np.tile(np.arange(plan.A, plan.tiles), plan.b)).all(), tag
            assert (np.diff(w[:n_a, 4]) >= 0).all() and (np.diff(w[n_a:, 4]) >= 0).all(), tag
        else:           # XCD i % 8 works on a contiguous run of each class
            ids = np.arange(len(wg))[valid]
            key = w[:, 4].astype(np.int64) * plan.tiles + w[:, 0]   # chunk-major position inside a class
            for cls in (in_a, ~in_a):
                slots = ids[cls] // 8
                for x in range(8):
                    run = key[cls][ids[cls] % 8 == x]
                    assert (np.diff(run) > 0).all(), (tag, x)
                if cls.any() and (~cls).any() and cls is in_a:
                    assert slots.max() < (ids[~in_a] // 8).min(), tag   # whole columns are dealt first


@pytest.mark.parametrize("ty", (4, 8, 12))
@pytest.mark.parametrize("per_round", (8, 256))
def test_every_plan_covers_its_window_once_and_is_no_dearer_than_the_uniform_one(ty, per_round, monkeypatch):
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    two_class = 0
    for width in WIDTHS:
        for rows in ROWS:
            for fold in ((False, True) if may_fold(width, rows, ty) else (False,)):
                tiles = tiles_of(width, rows, ty, fold)
                for planes in PLANES:
                    for zc_limit in sorted({planes, min(planes, 100)}):
                        tag = f"{width} x {rows} x {planes}, {ty} rows, limit {zc_limit}, round {per_round}, fold {fold}"
                        plan = f3d.pair8_plan(width, rows, planes, ty, zc_limit, per_round, fold)
                        zc, cost, wgs = uniform_plan(tiles, planes, zc_limit, per_round)
                        assert plan.tiles == tiles and plan.cost <= cost, tag
                        assert plan.wgs == plan.A * plan.a + (tiles - plan.A) * plan.b, tag
                        assert 0 <= plan.A < tiles and 1 <= plan.zc_b <= zc_limit and (plan.A == 0 or 1 <= plan.zc_a <= zc_limit), tag
                        rounds = lambda n: -(-n // per_round)
                        if plan.A:
                            two_class += 1
                            assert plan.cost < cost and (plan.A * plan.a) % per_round == 0, tag   # a tie keeps the uniform plan
                            assert plan.cost == (rounds(plan.A * plan.a) * (plan.zc_a + EXTRA) +
                                                 rounds((tiles - plan.A) * plan.b) * (plan.zc_b + EXTRA)), tag
                        else:
                            assert (plan.zc_b, plan.cost, plan.wgs) == (zc, cost, wgs), tag
                        if tiles <= per_round:   # one round covers the level: nothing changes
                            assert plan.A == 0 and plan.zc_b == zc, tag
                        check_decode(width, rows, planes, ty, fold, plan, 0 if planes % 2 else 3, tag)
    assert two_class > 20   # the grid reaches both kinds of plan


@pytest.mark.parametrize("per_round", (8, 256))
def test_the_switch_gives_the_uniform_plan_exactly(per_round, monkeypatch):
    monkeypatch.setenv("F3D_PAIR8_PLAN", "0")
    for ty in (4, 8, 12):
        for width in WIDTHS:
            for rows in ROWS:
                for planes in PLANES:
                    for fold in ((False, True) if may_fold(width, rows, ty) else (False,)):
                        tiles = tiles_of(width, rows, ty, fold)
                        plan = f3d.pair8_plan(width, rows, planes, ty, planes, per_round, fold)
                        zc, cost, wgs = uniform_plan(tiles, planes, planes, per_round)
                        assert (plan.A, plan.a, plan.zc_a) == (0, 0, 0), (width, rows, planes, ty, fold)
                        assert (plan.b, plan.zc_b, plan.wgs, plan.cost) == (-(-planes // zc), zc, wgs, cost), (width, rows, planes, ty, fold)


def test_the_round_override_is_read_per_call(monkeypatch):
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.setenv("F3D_PAIR8_ROUND", "8")
    assert f3d.pair8_plan(100, 61, 10, 12) == f3d.pair8_plan(100, 61, 10, 12, per_round=8)
    monkeypatch.delenv("F3D_PAIR8_ROUND")
    assert f3d.pair8_plan(100, 61, 10, 12) == f3d.pair8_plan(100, 61, 10, 12, per_round=256)
    assert f3d.pair8_plan(100, 61, 10, 12, per_round=8).A > 0 and f3d.pair8_plan(100, 61, 10, 12).A == 0


@pytest.mark.parametrize("size, tiles, bound", ((439, 259, 459), (463, 293, 555), (487, 328, 648), (512, 344, 732)))
def test_the_top_levels_of_the_default_pyramid_cost_what_the_model_priced(size, tiles, bound, monkeypatch):
    """12-row tiles, 256 per round, the fold where the width asks for it (463 = 7 x 64 + 15): whole columns for the first 256 tiles, the
    remainder cut as finely as fills the machine.  The enumeration may find cheaper plans, never dearer ones."""
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    fold = may_fold(size, size, 12)
    plan = f3d.pair8_plan(size, size, size, 12, size, 256, fold)
    assert plan.tiles == tiles and plan.A > 0
    assert plan.cost <= bound, plan
    assert plan.cost >= -(-tiles * size // 256), plan   # the ideal T D / 256
    check_decode(size, size, size, 12, fold, plan, 0, f"{size}^3")


def test_levels_that_one_round_covers_keep_their_chunks(monkeypatch):
    """The levels of the default pyramid below 439 (T <= 256 with the rows the launcher picks): today's chunk length, whatever the switch says."""
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    for size in (24, 40, 64, 128, 200, 256, 300, 358, 377, 397, 418):
        for ty in (4, 8, 12):
            fold = may_fold(size, size, ty)
            tiles = tiles_of(size, size, ty, fold)
            if tiles > 256:
                continue
            monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
            plan = f3d.pair8_plan(size, size, size, ty, size, 256, fold)
            monkeypatch.setenv("F3D_PAIR8_PLAN", "0")
            assert plan == f3d.pair8_plan(size, size, size, ty, size, 256, fold)
            assert plan.A == 0 and plan.zc_b == uniform_plan(tiles, size, size, 256)[0], (size, ty)


# ---- the chunk limit of the solver launches (solver_chunk_limit in csrc/f3d_pair8_plan.h, through f3d_solver_chunk_limit) ----
# A chunk of c planes of a launch that reads `reach` halo planes on either side touches planes z0 - reach .. z1 - 1 + reach, and the
# kernels form (plane - lowest plane) * plane_bytes + an offset inside the plane in 32 unsigned bits: (c + 2 reach) * plane_bytes must
# not pass 2^32.  The reach of each mode, read from the kernels: k_sweep6 / k_phiksi6 one plane each way, k_pair8 / k_wpair8 / k_sweep7
# z0 - 2 .. z1 + 1, k_tri z0 - 3 .. z1 + 2.
REACHES = (1, 2, 3)


def plane_sizes():
    """4 KiB .. 2 GiB: every power of two, its neighbours that a pitch of 256 bytes allows, and the sizes around each threshold
    2^32 / n (n = 3 .. 17: where the clamp to one plane starts, and where one plane with a halo of 1, 2, 3 stops fitting)"""
    sizes = set()
    for e in range(12, 32):
        sizes.update((1 << e, (1 << e) + 256, (1 << e) - 256, 3 << (e - 1)))
    for n in range(3, 18):
        q = (1 << 32) // n
        sizes.update((q // 256 * 256 - 256, q // 256 * 256, q // 256 * 256 + 256, q, q + 1))
    sizes.update((8192 * 32768, 16384 * 32768, 1664 * 262144, 1665 * 262144))   # planes of 256 and 512 MiB, 416 MiB and one row more
    return sorted(s for s in sizes if 4096 <= s <= 1 << 31)


@pytest.mark.parametrize("reach", REACHES)
def test_a_chunk_and_its_halo_never_pass_4_gib_or_the_launch_is_refused(reach):
    refused = fitted = 0
    for pb in plane_sizes():
        limit = f3d.solver_chunk_limit(pb, reach)
        one_fits = (1 + 2 * reach) * pb <= 1 << 32
        if limit == 0:
            assert not one_fits, (pb, reach)         # refused only where not even one plane fits
            refused += 1
            continue
        fitted += 1
        assert limit >= 1 and one_fits, (pb, reach, limit)
        assert (limit + 2 * reach) * pb <= 1 << 32, (pb, reach, limit)
        # as it always was where eight planes of slack leave a plane: every plan of every earlier container stays what it was
        if (0xffffffff // pb) - 8 >= 1:
            assert limit == min((0xffffffff // pb) - 8, 0x3fffffff), (pb, reach, limit)
        else:
            assert limit == 1, (pb, reach, limit)
    assert refused and fitted, "both sides of the threshold are among the sizes"


def test_where_the_chunk_limit_starts_to_refuse():
    gib = 1 << 30
    assert f3d.solver_chunk_limit(8192 * 32768, 2) == 7              # planes of 256 MiB: 15 - 8
    assert [f3d.solver_chunk_limit(gib // 2, r) for r in REACHES] == [1, 1, 1]   # 512 MiB: 7 planes are 3.5 GiB
    assert [f3d.solver_chunk_limit(gib, r) for r in REACHES] == [1, 0, 0]        # 1 GiB: 3 planes fit, 5 and 7 do not
    assert [f3d.solver_chunk_limit(2 * gib, r) for r in REACHES] == [0, 0, 0]
    for r in REACHES:   # the last plane size that fits and the first that does not, in steps of the 256-byte pitch unit
        edge = (1 << 32) // (1 + 2 * r) // 256 * 256
        assert f3d.solver_chunk_limit(edge, r) == 1 and f3d.solver_chunk_limit(edge + 256, r) == 0
    assert f3d.solver_chunk_limit(0, 1) == 0 and f3d.solver_chunk_limit(4096, -1) == 0
    assert f3d.solver_chunk_limit((1 << 32) + 256, 0) == 0
    assert f3d.solver_chunk_limit(4096, 3) == 0xffffffff // 4096 - 8
