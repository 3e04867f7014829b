"""The wide plan of a fused solver launch (csrc/f3d_pair8_plan.h: up to three classes of tiles, also on levels one round covers),
without a GPU: the plan through f3d_pair8_plan_wide -- the function the launcher calls -- and the kernel's own decode of a workgroup
number through f3d_pair8_decode_wide.

The cost formula is restated here: a class of `tiles` tiles in `chunks` chunks of `zc` planes costs ceil(tiles x chunks / per_round)
x (zc + 7) plane steps, a plan the sum over its classes.  "Never dearer than the parent's plan" is checked against f3d.pair8_plan,
which the existing tests pin."""
import importlib

import numpy as np
import pytest

f3d = importlib.import_module("cuda-flow3d_amd")

EXTRA = 7   # steps a chunk costs beside its planes (F3D_PAIR8_CHUNK_STEPS is not set in the suite)

WIDTHS = (64, 65, 96, 130, 200, 439, 600)
ROWS = (1, 13, 61, 200, 520)
PLANES = (1, 2, 3, 7, 13, 103, 439, 520)

# 12-row tiles, 256 per round, chunk limit = planes: size -> bound on the cost
PRICED = {263: 118, 277: 140, 307: 171, 323: 203, 340: 227, 358: 275, 377: 298, 397: 370, 418: 423, 463: 552, 487: 646, 512: 713}
UNCHANGED = (238, 250, 292, 439)
PRICED_TOTAL = 714716


def tiles_of(width, rows, ty, fold):
    ntx, nty = -(-width // 64), -(-rows // ty)
    return (ntx - 1) * nty + (nty + 1) // 2 if fold else ntx * nty


def may_fold(width, rows, ty):
    return 1 <= width % 64 <= 32 and width > 64 and rows > ty


def cost_of(classes, per_round):
    return sum(-(-t * c // per_round) * (zc + EXTRA) for t, c, zc in classes)


def classes_of_parent(p):
    """the classes of a Pair8Plan (f3d.pair8_plan), empty ones left out"""
    return tuple(c for c in ((p.A, p.a, p.zc_a), (p.tiles - p.A, p.b, p.zc_b)) if c[0])


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
    assert len(places) == plan.tiles == sum(c[0] for c in plan.classes), tag
    assert plan.wgs == sum(t * c for t, c, _ in plan.classes), tag
    first = np.cumsum([0] + [c[0] for c in plan.classes])        # first tile of each class
    cls_of_tile = np.repeat(np.arange(len(plan.classes)), [c[0] for c in plan.classes])
    zc_of_tile = np.repeat([c[2] for c in plan.classes], [c[0] for c in plan.classes])
    for remap in (0, 1):
        wg = f3d.pair8_decode_wide(width, rows, ty, fold, plan, remap, z_lo, z_lo + planes)
        valid = wg[:, 0] >= 0
        assert (wg[~valid] == -1).all(), tag
        assert int(valid.sum()) == plan.wgs, (tag, remap)
        # only an XCD's run is padded, by less than eight numbers per class
        pad = sum(-(t * c) % 8 for t, c, _ in plan.classes) if remap else 0
        assert len(wg) - plan.wgs == pad, (tag, remap, len(wg))
        w = wg[valid]
        # no workgroup without planes, every chunk inside the window and within its class's chunk length
        assert (w[:, 5] > w[:, 4]).all() and (w[:, 4] >= z_lo).all() and (w[:, 5] <= z_lo + planes).all(), (tag, remap)
        assert (w[:, 5] - w[:, 4] <= zc_of_tile[w[:, 0]]).all(), (tag, remap)
        assert (w[:, 1:4] == places[w[:, 0]]).all(), (tag, remap)
        # every (tile, plane) exactly once
        cover = np.zeros((plan.tiles, planes + 1), np.int64)
        np.add.at(cover, (w[:, 0], w[:, 4] - z_lo), 1)
        np.add.at(cover, (w[:, 0], w[:, 5] - z_lo), -1)
        assert (np.cumsum(cover, axis=1)[:, :planes] == 1).all(), (tag, remap)
        cls = cls_of_tile[w[:, 0]]
        if not remap:   # the classes in order, each chunk-major with tiles x first
            assert (np.diff(cls) >= 0).all(), tag
            for i, (t, c, zc) in enumerate(plan.classes):
                mine = w[cls == i]
                assert (mine[:, 0] == np.tile(np.arange(first[i], first[i] + t), c)).all(), (tag, i)
                assert (mine[:, 4] == z_lo + np.repeat(np.arange(c), t) * zc).all(), (tag, i)
        else:           # XCD i % 8 works on a contiguous run of each class, the classes in order
            ids = np.arange(len(wg))[valid]
            slot_end = -1
            for i, (t, c, zc) in enumerate(plan.classes):
                sel = cls == i
                key = (w[sel, 4].astype(np.int64) - z_lo) // zc * t + (w[sel, 0] - first[i])   # chunk-major position in the class
                per = -(-t * c // 8)
                assert (key == (ids[sel] % 8) * per + (ids[sel] // 8 - (slot_end + 1))).all(), (tag, i)
                assert (ids[sel] // 8).min() == slot_end + 1, (tag, i)
                slot_end += per


def check_plan(plan, parent, tiles, zc_limit, per_round, tag):
    """what holds for every plan of the launcher under the default switch"""
    assert plan.tiles == tiles and 1 <= len(plan.classes) <= 3, tag
    assert all(t >= 1 and c >= 1 and 1 <= zc <= zc_limit for t, c, zc in plan.classes), tag
    assert all((t * c) % per_round == 0 for t, c, _ in plan.classes[:-1]), tag   # every class but the last fills whole rounds
    assert plan.cost == cost_of(plan.classes, per_round), tag
    assert plan.cost <= parent.cost, tag
    if plan.cost == parent.cost:   # a tie keeps the parent's plan
        assert plan.classes == classes_of_parent(parent) and plan.wgs == parent.wgs, tag


@pytest.mark.parametrize("ty", (4, 8, 12))
@pytest.mark.parametrize("per_round", (8, 256))
def test_every_wide_plan_covers_its_window_once_and_is_no_dearer_than_the_parents(ty, per_round, monkeypatch):
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    kinds = {1: 0, 2: 0, 3: 0}
    cheaper = small_and_cheaper = 0
    for width in WIDTHS:
        for rows in ROWS:
            for fold in ((False, True) if may_fold(width, rows, ty) else (False,)):
                tiles = tiles_of(width, rows, ty, fold)
                for planes in PLANES:
                    for zc_limit in sorted({planes, min(planes, 100)}):
                        tag = f"{width} x {rows} x {planes}, {ty} rows, limit {zc_limit}, round {per_round}, fold {fold}"
                        plan = f3d.pair8_plan_wide(width, rows, planes, ty, zc_limit, per_round, fold)
                        parent = f3d.pair8_plan(width, rows, planes, ty, zc_limit, per_round, fold)
                        check_plan(plan, parent, tiles, zc_limit, per_round, tag)
                        kinds[len(plan.classes)] += 1
                        cheaper += plan.cost < parent.cost
                        small_and_cheaper += plan.cost < parent.cost and tiles <= per_round
                        check_decode(width, rows, planes, ty, fold, plan, 0 if planes % 2 else 3, tag)
    # the grid reaches every kind of plan, and levels one round covers are planned like any other
    assert min(kinds.values()) > 5 and cheaper > 20, (kinds, cheaper)
    assert small_and_cheaper > (0 if per_round == 8 else 5), small_and_cheaper


@pytest.mark.parametrize("size", sorted(PRICED) + list(UNCHANGED))
def test_the_default_pyramid_costs_what_the_model_priced(size, monkeypatch):
    """12-row tiles, 256 per round, the fold where the width asks for it.  The enumeration may find cheaper plans, never dearer ones."""
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    fold = may_fold(size, size, 12)
    tiles = tiles_of(size, size, 12, fold)
    plan = f3d.pair8_plan_wide(size, size, size, 12, size, 256, fold)
    parent = f3d.pair8_plan(size, size, size, 12, size, 256, fold)
    check_plan(plan, parent, tiles, size, 256, f"{size}^3")
    assert plan.cost >= -(-tiles * size // 256), plan   # the ideal T D / 256
    if size in PRICED:
        assert plan.cost <= PRICED[size], plan
    else:
        assert plan.classes == classes_of_parent(parent) and plan.cost == parent.cost, plan
    check_decode(size, size, size, 12, fold, plan, 0, f"{size}^3")


def test_the_priced_total_of_the_default_pyramid(monkeypatch):
    """The 40 levels of a 512^3 pyramid (sizes as GetLevel forms them), each at the rows per tile whose cost x step weight is lowest
    (80 / 100 / 128 for 4 / 8 / 12 rows, as pair8_rows weighs them)."""
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    total = total_parent = 0
    for level in range(40):
        size = f3d.level_geometry(512, 512, 512, 0.95, level)[0][0]   # ceil(512 x float pow(0.95f, level))
        assert abs(size - 512 * 0.95 ** level) < 1.001, (level, size)
        best = best_parent = None
        for ty, weight in ((4, 80), (8, 100), (12, 128)):
            fold = may_fold(size, size, ty)
            c = f3d.pair8_plan_wide(size, size, size, ty, size, 256, fold).cost * weight
            p = f3d.pair8_plan(size, size, size, ty, size, 256, fold).cost * weight
            best = c if best is None else min(best, c)
            best_parent = p if best_parent is None else min(best_parent, p)
        total += best
        total_parent += best_parent
    assert total_parent == 733148   # the figure the bound was priced against
    assert total <= PRICED_TOTAL, total


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("F3D_PAIR8_ROUND", raising=False)
    seen = 0
    for args in ((307, 307, 307, 12, 307, 256, False), (512, 512, 512, 12, 512, 256, False), (170, 12, 20, 4, 20, 16, True),
                 (100, 25, 38, 4, 38, 8, False), (463, 463, 463, 12, 100, 256, True), (100, 61, 10, 12, 10, 8, False)):
        tiles = tiles_of(args[0], args[1], args[3], args[6])
        monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
        wide = f3d.pair8_plan_wide(*args)
        parent = f3d.pair8_plan(*args)
        monkeypatch.setenv("F3D_PAIR8_PLAN", "2")
        assert f3d.pair8_plan_wide(*args) == wide, args
        monkeypatch.setenv("F3D_PAIR8_PLAN", "1")
        one = f3d.pair8_plan_wide(*args)
        assert (one.classes, one.cost, one.wgs, one.tiles) == (classes_of_parent(parent), parent.cost, parent.wgs, parent.tiles), args
        monkeypatch.setenv("F3D_PAIR8_PLAN", "0")
        zero = f3d.pair8_plan_wide(*args)
        assert len(zero.classes) == 1 and zero.classes[0][0] == tiles, args
        # the uniform plan: the first cheapest of 1 .. planes chunks within the limit
        planes, zc_limit, per_round = args[2], args[4], args[5]
        costs = {}
        for n in range(1, planes + 1):
            zc = -(-planes // n)
            if zc <= zc_limit:
                costs.setdefault(zc, cost_of(((tiles, -(-planes // zc), zc),), per_round))
        zc = min(costs, key=lambda z: (costs[z], -z))
        assert zero.classes[0] == (tiles, -(-planes // zc), zc) and zero.cost == costs[zc], args
        monkeypatch.delenv("F3D_PAIR8_PLAN")
        assert f3d.pair8_plan_wide(*args) == wide, args
        seen += wide.cost < parent.cost
    assert seen >= 4


def test_the_round_override_is_read_per_call(monkeypatch):
    monkeypatch.delenv("F3D_PAIR8_PLAN", raising=False)
    monkeypatch.setenv("F3D_PAIR8_ROUND", "8")
    assert f3d.pair8_plan_wide(100, 25, 38, 4) == f3d.pair8_plan_wide(100, 25, 38, 4, per_round=8)
    assert f3d.pair8_plan_wide(100, 25, 38, 4).classes == ((8, 1, 38), (4, 2, 19), (2, 4, 10))
    monkeypatch.delenv("F3D_PAIR8_ROUND")
    assert f3d.pair8_plan_wide(100, 25, 38, 4) == f3d.pair8_plan_wide(100, 25, 38, 4, per_round=256)
    assert f3d.pair8_plan_wide(100, 25, 38, 4) != f3d.pair8_plan_wide(100, 25, 38, 4, per_round=8)
