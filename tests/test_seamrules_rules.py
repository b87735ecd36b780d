"""The seam-tour rules under precedences and one-way seams, on the CPU: the restatement's scalar form (apply the move, test the
state) against its array form (the position limits the device uses), admissibility of every state of every descent, the exact programme
against brute force, the repair, and that the constraints of the GPU tests' cases bite."""
import numpy as np
import pytest

import seamrules_ref as S
import seamtour_ref as R


def euclid(m, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 10, (2 * m, 3)) * scale
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def hops(m, seed, hi=6):
    rs = np.random.RandomState(seed)
    d = rs.randint(1, hi, (2 * m, 2 * m)).astype(np.float64)
    return np.triu(d, 1) + np.triu(d, 1).T


@pytest.mark.parametrize("m,closed", [(2, True), (2, False), (3, True), (3, False), (4, True), (5, False), (6, True), (7, False), (9, True)])
def test_scalar_pass_equals_array_pass(m, closed):
    for seed in range(6):
        b, a, fx = S.random_rules(m, 10 * m + seed, closed)
        ru = S.Rules(m, closed, b, a, fx)
        W = R.quantise(hops(m, seed, 4) if seed & 1 else euclid(m, seed), m, closed)
        for r in range(1, 4):
            E = S.repair(R.random_start(ru.M, 77 + seed, r), ru)
            assert S.admissible(E, ru)
            for or_len in (0, 1, 3):
                assert S.best_move(E, W, or_len, ru) == S.best_move_scalar(E, W, or_len, ru), (seed, r, or_len, E)


def test_a_successor_inside_the_block_does_not_hold_it():
    """seams 1 -> 2 stand side by side: as a block they may jump forward past anything, a per-position minimum would stop them at once"""
    ru = S.Rules(5, True, [1], [2])
    E = [0, 2, 4, 6, 8]
    W = R.quantise(euclid(5, 3), 5)
    got = {num for num, kind, args in S.moves(5, 3) if S.admissible(R.move_apply(E, kind, args), ru)}
    assert 25 + (((1 * 3 + 1) * 5 + 4) * 2 + 0) in got and 25 + (((1 * 3 + 1) * 5 + 4) * 2 + 1) not in got
    assert 25 + (((1 * 3 + 0) * 5 + 2) * 2 + 0) not in got   # seam 1 alone may not pass seam 2
    assert S.best_move(E, W, 3, ru) == S.best_move_scalar(E, W, 3, ru)


def test_every_state_of_every_descent_is_admissible():
    n = 0
    for case in range(12):
        m, closed = 4 + case % 7, bool(case & 1)
        b, a, fx = S.random_rules(m, 500 + case, closed)
        trace = []
        r = S.seam_tour_rules(euclid(m, case), m, b, a, fx, closed=closed, n_starts=4, seed=case, trace=trace)
        assert all(S.admissible(E, r["rules"]) for E in trace)
        assert S.check(m, closed, b, a, fx, r["order"], r["dir"]) == (0, 0)
        n += len(trace)
    assert n > 100


@pytest.mark.parametrize("M", range(1, 8))
def test_exact_equals_brute_force(M):
    for closed in (True, False):
        m = M if closed else M - 1
        if m < 1:
            continue
        for seed in range(3):
            d = euclid(m, 40 + seed) if seed else hops(m, 40, 3)
            b, a, fx = S.random_rules(m, 90 + M + seed, closed)
            x = S.seam_tour_rules_exact(d, m, b, a, fx, closed)
            assert x["cost_q"] == S.brute_force_rules(d, m, b, a, fx, closed)
            assert S.admissible(x["E"], x["rules"]) and R.tour_cost(x["E"], x["W"]) == x["cost_q"]
            s = S.seam_tour_rules(d, m, b, a, fx, closed=closed, n_starts=3)
            assert s["cost_q"] >= x["cost_q"]
            # without rules the optimum is the old programme's
            assert S.seam_tour_rules_exact(d, m, closed=closed)["cost_q"] == R.seam_tour_exact(d, m, closed)["cost_q"]


def test_repair_keeps_an_admissible_draw():
    for case in range(10):
        m, closed = 5 + case, bool(case & 1)
        b, a, fx = S.random_rules(m, case, closed)
        ru = S.Rules(m, closed, b, a, fx)
        E = S.repair(R.random_start(ru.M, 5, case + 1), ru)
        assert S.admissible(E, ru) and S.repair(E, ru) == E
    ru = S.Rules(6, False)   # no rules: only the anchor moves to the front
    E = R.random_start(7, 3, 2)
    assert S.repair(E, ru) == [e for e in E if e >> 1 == 6] + [e for e in E if e >> 1 != 6]


def test_refused_rules():
    for kw in (dict(before=[0], after=[0]), dict(before=[0, 1], after=[1, 0]), dict(before=[1], after=[0]), dict(before=[5], after=[0]),
               dict(before=[-1], after=[2]), dict(fixed=[0, 3, 0, 0]), dict(before=[1, 2, 3], after=[2, 3, 1])):
        with pytest.raises(ValueError):
            S.Rules(4, True, **kw)
    S.Rules(4, False, [1], [0])   # an open tour may put any seam behind another


def test_the_constraints_bite():
    """a condition on the inputs: on the recipe the GPU tests use, the unconstrained tour breaks a rule in at least half of the cases"""
    broken = 0
    for case in range(24):
        m, closed = 5 + case % 16, bool(case & 1)
        d = euclid(m, 700 + case)
        b, a, fx = S.random_rules(m, 700 + case, closed)
        free = R.seam_tour(d, m, closed=closed, n_starts=2, seed=case)
        broken += S.check(m, closed, b, a, fx, free["order"], free["dir"]) != (0, 0)
    assert broken >= 12, broken
