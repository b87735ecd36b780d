"""The rules of the seam-tour definition, checked on the numpy restatement alone (tests/seamtour_ref.py): no product
code, no device.  Seeded Euclidean endpoint sets and small-integer hop-like matrices (which force equal-cost ties)."""
import itertools

import numpy as np
import pytest

import seamtour_ref as R


def euclid(m, seed, dim=3):
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 10, (2 * m, dim))
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def hops(m, seed, hi=6):
    rs = np.random.RandomState(seed)
    d = rs.randint(1, hi, (2 * m, 2 * m)).astype(np.float64)
    return np.triu(d, 1) + np.triu(d, 1).T


CASES = [(kind, m, seed) for kind in (euclid, hops) for m, seed in ((2, 1), (3, 2), (5, 3), (8, 4), (12, 5), (20, 6))]


@pytest.mark.parametrize("kind,m,seed", CASES)
@pytest.mark.parametrize("closed", [True, False])
def test_returned_cost_is_the_cost_of_the_returned_tour(kind, m, seed, closed):
    d = kind(m, seed)
    r = R.seam_tour(d, m, closed=closed, n_starts=3, seed=seed)
    W = R.quantise(d, m, closed)
    E = [2 * int(s) + int(x) for s, x in zip(r["order"], r["dir"])]
    if closed:
        assert R.tour_cost(E, W) == r["cost_q"]
        assert r["order"][0] == 0
    else:   # open: the travel between consecutive seams, nothing for the way back
        assert sum(int(W[E[k] ^ 1, E[k + 1]]) for k in range(m - 1)) == r["cost_q"]
    assert sorted(r["order"].tolist()) == list(range(m))
    assert r["cost_q"] == r["start_cost_q"].min() == r["start_cost_q"][r["summary"]["best_start"]]


@pytest.mark.parametrize("M", range(1, 10))
def test_every_delta_is_the_cost_difference_of_applying_the_move(M):
    for kind in (euclid, hops):
        W = R.quantise(kind(M, 10 + M), M)
        E = R.random_start(M, 77, 1 + M)
        c0 = R.tour_cost(E, W)
        all_moves = R.moves(M, 3)
        assert len({num for num, _, _ in all_moves}) == len(all_moves)
        for num, k, args in all_moves:
            assert R.decode(num, M) == (k, args)
            E2 = R.move_apply(E, k, args)
            assert sorted(x >> 1 for x in E2) == list(range(M))
            assert R.tour_cost(E2, W) - c0 == R.move_delta(E, W, k, args), (M, k, args)
        for or_len in range(4):   # the whole-pass form picks what the scalar form picks
            want = R.best_move_scalar(E, W, or_len)
            assert R.best_move(E, W, or_len) == want
        if M == 1:
            assert all_moves == []


@pytest.mark.parametrize("kind,m,seed", CASES)
def test_an_uncapped_result_admits_no_improving_move_and_costs_are_ordered(kind, m, seed):
    d = kind(m, seed)
    for closed, or_len in itertools.product((True, False), (0, 1, 3)):
        r = R.seam_tour(d, m, closed=closed, or_len=or_len, n_starts=4, seed=5)
        s = r["summary"]
        assert s["n_capped"] == 0
        for num, k, args in R.moves(len(r["E"]), or_len):
            assert R.move_delta(r["E"], r["W"], k, args) >= 0
        assert s["cost_q"] <= s["start0_cost_q_out"] <= s["start0_cost_q_in"]
        assert s["passes_total"] == r["start_passes"].sum()


def test_max_passes_ends_a_start_and_counts_it():
    d = euclid(20, 9)
    full = R.seam_tour(d, 20, n_starts=2, seed=3)
    assert full["start_passes"].min() > 3
    cut = R.seam_tour(d, 20, n_starts=2, seed=3, max_passes=3)
    assert cut["summary"]["n_capped"] == 2 and cut["start_passes"].tolist() == [3, 3]
    assert cut["cost_q"] > full["cost_q"]
    # a cap equal to the passes a start takes (its last pass finds nothing) is not counted
    exact = R.seam_tour(d, 20, n_starts=1, max_passes=int(full["start_passes"][0]))
    assert exact["summary"]["n_capped"] == 0 and exact["cost_q"] == full["start_cost_q"][0]


@pytest.mark.parametrize("m,closed", [(m, True) for m in range(1, 8)] + [(m, False) for m in range(1, 7)])
def test_exact_equals_brute_force(m, closed):
    M = m if closed else m + 1
    for kind in (euclid, hops):
        d = kind(m, 20 + M)
        ex = R.seam_tour_exact(d, m, closed)
        assert ex["cost_q"] == R.brute_force(d, m, closed)
        assert R.tour_cost(ex["E"], ex["W"]) == ex["cost_q"]
        assert ex["E"][0] == 0 and sorted(x >> 1 for x in ex["E"]) == list(range(M))


@pytest.mark.parametrize("kind,m,seed", [c for c in CASES if c[1] <= 12])
@pytest.mark.parametrize("closed", [True, False])
def test_exact_bounds_the_search_and_is_a_fixed_point_of_it(kind, m, seed, closed):
    d = kind(m, seed)
    ex = R.seam_tour_exact(d, m, closed)
    for or_len in (0, 3):
        r = R.seam_tour(d, m, closed=closed, or_len=or_len, n_starts=3, seed=seed)
        assert (ex["cost_q"] <= r["start_cost_q"]).all()
    again = R.seam_tour(d, m, closed=closed, order0=ex["order"], dir0=ex["dir"])
    assert again["cost_q"] == ex["cost_q"] == again["summary"]["start0_cost_q_in"]
    assert again["start_passes"].tolist() == [1]


@pytest.mark.parametrize("n", [3, 5, 7])
def test_seams_whose_ends_coincide_reduce_to_a_plain_tsp(n):
    rs = np.random.RandomState(n)
    p = rs.uniform(0, 10, (n, 2))
    d1 = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    d = np.repeat(np.repeat(d1, 2, 0), 2, 1)
    w1 = np.rint(d1 * R.Q).astype(np.int64)
    tsp = min(sum(int(w1[a, b]) for a, b in zip((0,) + q, q + (0,))) for q in itertools.permutations(range(1, n)))
    assert R.seam_tour_exact(d, n)["cost_q"] == tsp
    assert R.seam_tour(d, n, n_starts=8)["cost_q"] >= tsp


@pytest.mark.parametrize("kind,m,seed", [(euclid, 6, 31), (hops, 9, 32)])
def test_the_open_result_is_the_dummy_construction_done_by_hand(kind, m, seed):
    d = kind(m, seed)
    big = np.zeros((2 * m + 2, 2 * m + 2))
    big[:2 * m, :2 * m] = d   # a real seam m whose two ends cost nothing to reach
    kw = dict(or_len=3, n_starts=3, seed=seed)
    op = R.seam_tour(d, m, closed=False, **kw)
    cl = R.seam_tour(big, m + 1, closed=True, **kw)
    assert op["E"] == cl["E"] and op["cost_q"] == cl["cost_q"]
    assert np.array_equal(op["start_cost_q"], cl["start_cost_q"]) and np.array_equal(op["start_passes"], cl["start_passes"])
    at = cl["E"].index(2 * m) if 2 * m in cl["E"] else cl["E"].index(2 * m + 1)
    rot = [cl["E"][(at + 1 + k) % (m + 1)] for k in range(m)]
    assert op["order"].tolist() == [x >> 1 for x in rot] and op["dir"].tolist() == [x & 1 for x in rot]
    ex_o, ex_c = R.seam_tour_exact(d, m, closed=False), R.seam_tour_exact(big, m + 1, closed=True)
    assert ex_o["cost_q"] == ex_c["cost_q"] and ex_o["E"] == ex_c["E"]


def test_bad_costs_and_starts_are_refused():
    d = euclid(4, 1)
    for bad in (-1.0, np.nan, np.inf, float(1 << 20)):
        e = d.copy()
        e[1, 5] = bad
        with pytest.raises(ValueError):
            R.quantise(e, 4)
    e = d.copy()
    e[5, 1] = np.nan   # below the diagonal, on it and inside a seam: never read
    e[2, 2] = -1
    e[2, 3] = np.inf
    assert np.array_equal(R.quantise(e, 4), R.quantise(d, 4))
    with pytest.raises(ValueError):
        R.seam_tour(d, 4, order0=[0, 1, 1, 2])
    with pytest.raises(ValueError):
        R.seam_tour(d, 4, dir0=[0, 1, 2, 0])
