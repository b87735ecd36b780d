"""What the seam ordering does on degenerate distance matrices, asserted on the C oracle (CPU): the behaviour the GPU
kernels are held to in tests/test_gpu_gtsp_dispatch.py.  Where the compiled reference is present
(oracle/_ref/ref_harness), the same graphs also go through the reference itself."""
import os

import numpy as np
import pytest

import oracle_lib as O
import waf
from tmpw import TMPW

INF = float(0x3f3f3f3f)   # ACS_GTSP.hpp:19


def closed_chain(n):
    """the tour 0 -> 1 -> ... -> n-1 -> 0 as (r, s) edges"""
    a = np.arange(n, dtype=np.int32)
    return np.stack([a, np.roll(a, -1)], 1)


@pytest.mark.parametrize("n", [2, 3, 5, 64])
@pytest.mark.parametrize("cnt", [None, 1])
def test_coincident_cities(n, cnt):
    """every seam at one point: pheromone_0 = cnt / 0 = +inf, so every term of the roulette is +inf and each ant takes
    its first unvisited city; all tours cost 0, the first one is kept, and the run stops on stagnation (n + 1
    non-improving iterations after the first)"""
    for mode, kw in ((O.DEV, dict(seed=5, stream=1)), (O.REF, dict(rng=O.srand(3)))):
        o = O.gtsp_solve(np.zeros((n, n)), cnt=cnt, mode=mode, want_pher=True, **kw)
        assert o["iters"] == n + 2 and o["L"] == 0.0
        assert np.array_equal(o["edges"], closed_chain(n))
        assert np.all(np.isposinf(o["pher"]))


@pytest.mark.parametrize("n", [2, 3, 5, 64])
def test_coincident_cities_cnt0(n):
    """cnt = 0: pheromone_0 = 0 / 0 = NaN, no ant ever picks a city (the roulette compares against NaN), each stays
    at its start; in REF mode it then draws at EVERY step, n*n libc values per iteration instead of n*(n-1)"""
    rng = O.srand(3)
    o = O.gtsp_solve(np.zeros((n, n)), cnt=0, mode=O.REF, rng=rng, want_pher=True)
    assert o["iters"] == n + 2 and o["L"] == 0.0
    assert not o["edges"].any()
    assert np.all(np.isnan(o["pher"]))
    assert rng.calls == o["iters"] * n * n


def test_draw_count_of_a_normal_run():
    """every ant picks a city at steps 0..n-2 and none at the last: n*(n-1) libc draws per iteration, the count the
    GPU kernels replay (k_gtsp, k_gtsp_fast, k_gtspw_*)"""
    rs = np.random.RandomState(4)
    for n, d in ((17, rs.uniform(0.1, 1, (17, 17))), (9, np.zeros((9, 9))), (12, np.round(rs.uniform(0, 1, (12, 12)), 1))):
        rng = O.srand(n)
        o = O.gtsp_solve(d, mode=O.REF, rng=rng, max_iterations=30)
        assert rng.calls == o["iters"] * n * (n - 1), n


@pytest.mark.parametrize("n", [3, 20])
def test_above_inf_never_improves(n):
    """all tours cost more than the INF sentinel: no best tour is ever recorded (edges stay 0, the cost stays INF), no
    deposit happens, and the run stops after n + 1 iterations with pheromone_0 * 0.9^(n+1) everywhere"""
    rs = np.random.RandomState(n)
    d = 2e9 + rs.uniform(0, 1e9, (n, n))
    np.fill_diagonal(d, 0.0)
    cnt = n * (n - 1) // 2
    o = O.gtsp_solve(d, mode=O.DEV, seed=1, stream=0, want_pher=True)
    assert o["iters"] == n + 1 and o["L"] == INF and not o["edges"].any()
    tmp = 0.0
    for i in range(n):
        for j in range(i + 1, n):
            tmp += d[i, j]
    p = cnt / (tmp * n)
    for _ in range(n + 1):
        p *= 0.9
    assert np.all(o["pher"] == p)


def test_overflow_and_underflow_scales():
    """1e-300: pheromone_0 (~1e299) * h^6 (~1e48) = +inf, the roulette picks the first unvisited city; 1e150: h^6
    underflows to 0, the roulette sums 0 and takes the first unvisited city too, and every tour is above INF"""
    rs = np.random.RandomState(2)
    P = rs.uniform(0, 1, (12, 3))
    d = np.abs(P[:, None, :] - P[None, :, :]).sum(-1)
    o = O.gtsp_solve(d * 1e-300, mode=O.DEV, seed=1, stream=0, max_iterations=1, want_pher=True)
    k = int(o["edges"][0, 0])
    order = [k] + o["edges"][:-1, 1].tolist()
    assert order == [k] + [c for c in range(12) if c != k] and o["edges"][-1, 1] == k
    assert np.isfinite(o["L"]) and np.all(np.isfinite(o["pher"])) and o["pher"].max() > 1e298
    o = O.gtsp_solve(d * 1e150, mode=O.DEV, seed=1, stream=0, want_pher=True)
    assert o["iters"] == 13 and o["L"] == INF and not o["edges"].any()


# ------------------------------------------------------------------ the same graphs through the reference
def _graph(path, d, cnt):
    n = len(d)
    with open(path, "w") as f:
        f.write("%d %d\n" % (n, cnt))
        for a in range(n):
            for b in range(a + 1, n):
                f.write("%.17g\n" % d[a, b])


def _sym(rs, n, kind):
    if kind == "coincident":
        return np.zeros((n, n))
    if kind == "clusters":
        side = np.arange(n) % 3 == 0
        return np.where(side[:, None] == side[None, :], 0.0, 1.375)
    P = rs.randint(0, 4, (n, 3)).astype(np.float64)
    d = np.round(np.abs(P[:, None, :] - P[None, :, :]).sum(-1) / 7.0, 3)
    d = {"ties": d, "scale_1e-300": d * 1e-300 + 1e-300}[kind]
    np.fill_diagonal(d, 0.0)
    return d


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/ref_harness not built (needs the reference sources)")
@pytest.mark.parametrize("kind,cnt", [("coincident", None), ("coincident", 1), ("coincident", 0), ("clusters", None),
                                      ("ties", None), ("ties", 0), ("scale_1e-300", None)])
def test_degenerate_graphs_against_the_reference(kind, cnt):
    """(distances above INF are asserted on the oracle alone: when no tour ever beats INF, the reference reads its
    empty best tour and crashes)"""
    tmp = TMPW + "weld_gtsp_rules_%d" % os.getuid()
    os.makedirs(tmp, exist_ok=True)
    rs = np.random.RandomState(len(kind))
    for n in (3, 11):
        d = _sym(rs, n, kind)
        c = n * (n - 1) // 2 if cnt is None else cnt
        _graph(tmp + "/g.in", d, c)
        r = O.run_ref("gtsp", tmp + "/t.waf", graph=tmp + "/g.in", seed=n)
        dd = r["gtsp_dis"].reshape(n, n)
        assert np.array_equal(dd.view(np.uint64), d.view(np.uint64))
        rng = O.srand(n)
        o = O.gtsp_solve(dd, cnt=c, mode=O.REF, rng=rng, want_pher=True)
        tag = (kind, cnt, n)
        assert o["iters"] == waf.scalar(r, "gtsp_iters") and o["L"] == waf.scalar(r, "tour_L"), tag
        assert np.array_equal(o["edges"].reshape(-1), r["tour_edges"]), tag
        p, rp = o["pher"].reshape(-1), r["gtsp_pher"]
        assert np.array_equal(np.isnan(p), np.isnan(rp)), tag
        assert np.array_equal(p[~np.isnan(p)].view(np.uint64), rp[~np.isnan(rp)].view(np.uint64)), tag
        assert rng.calls == waf.scalar(r, "rand_calls") and O.rand(rng) == waf.scalar(r, "next_rand"), tag
