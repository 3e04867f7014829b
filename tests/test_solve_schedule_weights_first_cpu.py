"""The weights-first cut of an outer iteration's sweeps (host/solve_schedule.cpp: CutSweepsWeightsFirst, through
plan_sweeps_weights_first): pure host arithmetic, no device."""
import pytest


@pytest.mark.parametrize("K", range(1, 9))
def test_the_cut_covers_every_sweep_once_and_starts_with_the_weights(f3d, K):
    cut = f3d.plan_sweeps_weights_first(K)
    # every sweep exactly once: launch i starts where launch i-1 ended, the first at sweep 0, the last ends at K (the operator finds the
    # level's last launch by first + sweeps = K)
    covered = []
    for first, n, _, _ in cut:
        assert first == len(covered)
        covered += list(range(first, first + n))
    assert covered == list(range(K))
    assert cut[0] == (0, 1, True, False)                        # (P, S)
    assert all(not wf for _, _, wf, _ in cut[1:])
    assert all(not nxt for _, _, _, nxt in cut)                 # the weights are made where they are used
    assert all(n == 2 for _, n, _, _ in cut[1:-1])              # pairs ...
    if K > 1:
        assert cut[-1][1] == (1 if K % 2 == 0 else 2)           # ... and a single sweep for an even K
    assert len(cut) == 1 + K // 2


def test_no_sweeps_no_launches(f3d):
    assert f3d.plan_sweeps_weights_first(0) == []


@pytest.mark.parametrize("K", range(1, 9))
def test_the_other_cut_is_what_it_was(f3d, K):
    pairs = [2] * (K // 2) + [1] * (K % 2)
    for carry in (False, True):
        got = f3d.plan_sweeps(K, True, False, carry)
        assert [n for n, _ in got] == pairs
        assert [w for _, w in got] == [False] * (len(pairs) - 1) + [carry and K % 2 == 1]
        assert f3d.plan_sweeps(K, False, False, carry) == [(1, False)] * K
    assert f3d.plan_sweeps(5, True, True, True) == [(3, False), (2, True)]
