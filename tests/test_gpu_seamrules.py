"""wa_gtsp_seam_tour_rules / wa_gtsp_seam_tour_rules_exact on the device against the numpy restatement (tests/seamrules_ref.py), byte for
byte: order, direction, every start's cost and passes, the summary.  Seeded Euclidean endpoint sets and small-integer matrices
(equal-cost ties); rules by seamrules_ref.random_rules (m pairs oriented by a hidden order, a quarter of the seams one-way) unless a
case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import seamrules_ref as S
import seamtour_ref as R
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG, CAPACITY = 1, 7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def euclid(m, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 10, (2 * m, 3)) * scale
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def hops(m, seed, hi=6):
    rs = np.random.RandomState(seed)
    d = rs.randint(1, hi, (2 * m, 2 * m)).astype(np.float64)
    return np.triu(d, 1) + np.triu(d, 1).T


def rules_of(kind, m, seed, closed):
    """(before, after, fixed): 'r' the random recipe, 'n' none, 't' a total order (only flips remain), 'f' the recipe with every seam
    one-way, 'd' the recipe with every pair given twice"""
    b, a, fx = S.random_rules(m, seed, closed)
    if kind == "n":
        return None, None, None
    if kind == "t":
        rs = np.random.RandomState(seed)
        p = rs.permutation(m)
        if closed:
            p = np.concatenate([[0], p[p != 0]])
        return p[:-1].astype(np.int32), p[1:].astype(np.int32), fx
    if kind == "f":
        return b, a, np.random.RandomState(seed).randint(1, 3, m).astype(np.uint8)
    if kind == "d":
        return np.concatenate([b, b]), np.concatenate([a, a]), fx
    return b, a, fx


def given_start(m, seed, closed, b, a, fx):
    """an admissible order0 / dir0 that is not the repaired identity: a repaired random draw with the dummy dropped"""
    ru = S.Rules(m, closed, () if b is None else b, () if a is None else a, fx)
    E = [e for e in S.repair(R.random_start(ru.M, seed, 1), ru) if (e >> 1) < m]
    return np.array([e >> 1 for e in E], np.int32), np.array([e & 1 for e in E], np.uint8)


def same(got, want):
    assert np.array_equal(got["order"], want["order"]) and got["order"].dtype == np.int32
    assert np.array_equal(got["dir"], want["dir"]) and got["dir"].dtype == np.uint8
    assert got["cost_q"] == want["cost_q"]
    assert np.array_equal(got["start_cost_q"], want["start_cost_q"])
    assert np.array_equal(got["start_passes"], want["start_passes"])
    assert got["summary"] == want["summary"]


def kw_rules(b, a, fx):
    return dict(before=() if b is None else b, after=() if a is None else a, fixed=fx)


# (costs, m, scale / hi, closed, or_len, n_starts, rules, given start, max_passes)
BIG = 1 << 20
CASES = [
    # M = 2, 3, 4: where min(or_len, M - 2) and j - i <= M - 2 bite
    ("e", 1, 1, True, 3, 3, "n", False, BIG), ("e", 1, 1, False, 3, 4, "f", False, BIG), ("e", 2, 1, True, 3, 4, "r", False, BIG),
    ("h", 2, 3, False, 3, 4, "r", True, BIG), ("e", 3, 1, True, 3, 5, "r", False, BIG), ("h", 3, 3, False, 2, 5, "t", False, BIG),
    ("e", 4, 1, True, 3, 6, "r", True, BIG), ("e", 3, 1, False, 1, 6, "n", False, BIG),
    # the storage and team paths: narrow / wide W in LDS with a wavefront per descent (M <= 64), the workgroup above; narrow W in LDS up
    # to M = 100, in memory from 101; a wide W above 64 always in memory.  scale 1e4 gives costs above 2^32 quanta
    ("e", 16, 1e4, True, 3, 5, "r", False, BIG), ("e", 40, 1e4, False, 3, 3, "r", True, BIG), ("e", 64, 1, True, 3, 4, "r", False, BIG),
    ("e", 63, 1, False, 3, 4, "r", True, BIG), ("h", 64, 4, True, 3, 3, "n", False, BIG), ("e", 65, 1, True, 3, 3, "r", False, BIG),
    ("e", 64, 1, False, 3, 3, "r", False, BIG), ("e", 70, 1e4, True, 2, 2, "r", False, BIG), ("e", 100, 1, True, 3, 2, "r", True, BIG),
    ("e", 99, 1, False, 3, 2, "d", False, BIG), ("e", 101, 1, True, 3, 2, "r", False, BIG), ("h", 100, 5, False, 3, 2, "r", False, BIG),
    # a total order, every seam one-way, both, and caps that bind
    ("e", 12, 1, True, 3, 8, "t", False, BIG), ("h", 9, 4, False, 3, 8, "t", True, BIG), ("e", 14, 1, True, 3, 8, "f", False, BIG),
    ("e", 11, 1, False, 3, 8, "f", True, BIG), ("e", 18, 1, True, 3, 6, "r", False, 1), ("e", 18, 1, False, 3, 6, "r", False, 2),
    ("e", 70, 1, True, 3, 3, "r", False, 2),
]
# about 30 random cases, m = 5 .. 20, open and closed, every or_len, Euclidean and tied costs, some with a caller's start
CASES += [("h" if k % 3 == 2 else "e", 5 + k % 16, 3 + k % 3 if k % 3 == 2 else 1, bool(k & 1), (3, 3, 2, 1, 0)[k % 5], 4 + k % 7,
           "d" if k % 8 == 7 else "r", k % 4 == 3, BIG) for k in range(30)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_search_is_bit_equal_to_the_restatement(ctx, case):
    kind, m, par, closed, or_len, n_starts, rk, given, cap = CASES[case]
    d = euclid(m, 100 + case, par) if kind == "e" else hops(m, 100 + case, par)
    b, a, fx = rules_of(rk, m, 900 + case, closed)
    o0, d0 = given_start(m, case, closed, b, a, fx) if given else (None, None)
    kw = dict(closed=closed, or_len=or_len, n_starts=n_starts, seed=0xC0FFEE + case, order0=o0, dir0=d0, max_passes=cap)
    trace = []
    want = S.seam_tour_rules(d, m, trace=trace, **kw_rules(b, a, fx), **kw)
    got = api.seam_tour_rules(ctx, d, b, a, fx, **kw)
    same(got, want)
    assert all(S.admissible(E, want["rules"]) for E in trace)
    assert (want["summary"]["n_capped"] > 0) == (cap != BIG)
    assert got["cost_q"] <= got["summary"]["start0_cost_q_out"] <= got["summary"]["start0_cost_q_in"]
    if rk != "n":
        assert api.seam_rules_check(got["order"], got["dir"], b, a, fx, closed=closed, ctx=ctx) == (0, 0)
    again = api.seam_tour_rules(ctx, d, b, a, fx, **kw)   # the same bytes on every call
    for k in ("order", "dir", "start_cost_q", "start_passes"):
        assert got[k].tobytes() == again[k].tobytes()
    assert got["summary"] == again["summary"]


def test_more_starts_than_teams_are_resident(ctx):
    """m = 6 with 9000 starts: 256 CUs hold 8 workgroups of 4 descents each, so teams take a second start.  The restatement descends a
    sample of the starts (the first, the last, and those around 8192); the summary is held against the device's own per-start arrays"""
    m, closed, seed = 6, True, 4242
    d = euclid(m, 5)
    b, a, fx = S.random_rules(m, 17, closed)
    n = 9000
    got = api.seam_tour_rules(ctx, d, b, a, fx, closed=closed, n_starts=n, seed=seed)
    ru = S.Rules(m, closed, b, a, fx)
    W = R.quantise(d, m, closed)
    finals = {}
    for r in list(range(1, 40)) + list(range(8170, 8230)) + list(range(n - 40, n)):
        E, p, c = S.descend(S.repair(R.random_start(ru.M, seed, r), ru), W, 3, 1 << 20, ru)
        finals[r] = E
        assert (int(got["start_cost_q"][r]), int(got["start_passes"][r]), c) == (R.tour_cost(E, W), p, 0), r
    s = got["summary"]
    best = int(np.argmin(got["start_cost_q"]))
    assert (s["best_start"], s["cost_q"], s["passes_total"], s["n_capped"]) == (best, int(got["start_cost_q"][best]), int(got["start_passes"].sum()), 0)
    assert (s["n_prec"], s["n_fixed"], s["n_starts"]) == (ru.n_prec, ru.n_fixed, n)
    E = finals[best] if best in finals else S.descend(S.repair(R.random_start(ru.M, seed, best), ru) if best else S.start0(ru), W, 3, 1 << 20, ru)[0]
    order, dirs = R.emit(E, m, closed)
    assert np.array_equal(got["order"], order) and np.array_equal(got["dir"], dirs)
    assert got["start_cost_q"].min() >= api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)["cost_q"]


def test_refused_calls_leave_the_outputs_untouched(ctx):
    lib = ctx.lib
    m = 6
    good = euclid(m, 1)

    def call(dist=good, m=m, closed=1, or_len=3, n_starts=4, max_passes=100, before=(1, 2), after=(2, 3), fixed=(0, 1, 0, 2, 0, 0), n_prec=None,
             order0=None, dir0=None, null=()):
        dist = np.ascontiguousarray(dist, np.float64)
        p = L.SeamParams(closed, or_len, n_starts, max_passes, 5)
        order, dirs = np.full(16, -7, np.int32), np.full(16, 9, np.uint8)
        costs, passes = np.full(8, -7, np.int64), np.full(8, -7, np.int32)
        s = L.SeamRulesSummary()
        C.memset(C.byref(s), 0x5a, C.sizeof(s))
        was = bytes(s)
        b, a, f = np.array(before, np.int32), np.array(after, np.int32), np.array(fixed, np.uint8)
        ptr = lambda name, x: None if name in null else x.ctypes.data
        o0 = None if order0 is None else np.asarray(order0, np.int32)
        d0 = None if dir0 is None else np.asarray(dir0, np.uint8)
        rc = lib.wa_gtsp_seam_tour_rules(ctx.h, ptr("dist", dist), m, None if "params" in null else C.byref(p), ptr("before", b), ptr("after", a),
                                         len(b) if n_prec is None else n_prec, ptr("fixed", f), api._ptr(o0), api._ptr(d0), ptr("order", order),
                                         ptr("dir", dirs), costs.ctypes.data, passes.ctypes.data, None if "sum" in null else C.byref(s))
        untouched = (order == -7).all() and (dirs == 9).all() and (costs == -7).all() and (passes == -7).all() and bytes(s) == was
        return rc, bool(untouched)

    assert call() == (0, False)
    assert call(null=("fixed",))[0] == 0 and call(n_prec=0, null=("before", "after"))[0] == 0
    assert call(order0=[0, 1, 2, 3, 4, 5], dir0=[1, 0, 1, 1, 0, 1])[0] == 0
    assert call(closed=0, after=(2, 0))[0] == 0   # an open tour may put a seam before seam 0
    bad = [call(null=(n,)) for n in ("dist", "params", "order", "dir", "sum", "before", "after")]
    bad += [call(m=0), call(m=1025), call(or_len=-1), call(or_len=4), call(n_starts=0), call(n_starts=(1 << 20) + 1), call(max_passes=0),
            call(max_passes=(1 << 20) + 1), call(n_prec=-1), call(n_prec=65537),
            call(before=(1, 6)), call(before=(-1, 2)), call(after=(2, 6)), call(after=(2, -1)),         # a seam outside 0 .. m-1
            call(before=(1, 3)), call(before=(1, 2, 3), after=(2, 3, 1)), call(after=(2, 1)),           # before == after; cycles
            call(after=(2, 0)),                                                                        # nothing goes before seam 0 of a closed tour
            call(fixed=(0, 1, 0, 3, 0, 0)),
            call(order0=[0, 1, 2, 3, 4, 4]), call(order0=[0, 1, 2, 3, 4, 6]), call(dir0=[0, 0, 0, 1, 0, 2]),
            call(order0=[1, 0, 2, 3, 4, 5]),                                                           # a closed order0 starts with seam 0
            call(order0=[0, 2, 1, 3, 4, 5]), call(order0=[0, 1, 3, 2, 4, 5]),                           # order0 breaks a pair
            call(dir0=[0, 1, 0, 1, 0, 0]), call(order0=[0, 1, 2, 3, 4, 5], dir0=[0, 0, 0, 0, 0, 0])]    # dir0 breaks a one-way seam
    for v in (-1e-9, np.nan, np.inf, float(1 << 20)):
        e = good.copy()
        e[3, 8] = v
        bad.append(call(dist=e))
    for k, r in enumerate(bad):
        assert r == (ARG, True), k

    def exact(dist=good, m=m, closed=1, before=(1, 2), after=(2, 3), fixed=(0, 1, 0, 2, 0, 0), n_prec=None, null=()):
        dist = np.ascontiguousarray(dist, np.float64)
        order, dirs, cost = np.full(32, -7, np.int32), np.full(32, 9, np.uint8), np.full(1, -7, np.int64)
        b, a, f = np.array(before, np.int32), np.array(after, np.int32), np.array(list(fixed) + [0] * 32, np.uint8)
        ptr = lambda name, x: None if name in null else x.ctypes.data
        rc = lib.wa_gtsp_seam_tour_rules_exact(ctx.h, ptr("dist", dist), m, closed, ptr("before", b), ptr("after", a), len(b) if n_prec is None else n_prec,
                                               ptr("fixed", f), ptr("order", order), ptr("dir", dirs), ptr("cost", cost))
        return rc, bool((order == -7).all() and (dirs == 9).all() and (cost == -7).all())

    assert exact() == (0, False) and exact(null=("fixed",))[0] == 0
    bad = [exact(null=(n,)) for n in ("dist", "order", "dir", "cost", "before", "after")]
    bad += [exact(m=0), exact(n_prec=-1), exact(n_prec=65537), exact(before=(1, 6)), exact(after=(2, -1)), exact(before=(1, 3)), exact(after=(2, 1)),
            exact(after=(2, 0)), exact(fixed=(0, 1, 0, 3, 0, 0))]
    e = good.copy()
    e[0, 2] = -1
    bad.append(exact(dist=e))
    for k, r in enumerate(bad):
        assert r == (ARG, True), k
    assert exact(dist=euclid(17, 2), m=17) == (CAPACITY, True)
    assert exact(dist=euclid(16, 2), m=16, closed=0) == (CAPACITY, True)
    assert exact(dist=euclid(16, 2), m=16)[0] == 0 and exact(dist=euclid(15, 2), m=15, closed=0)[0] == 0


# 20 cases, M = 2 .. 12 (M, closed, rules)
EXACT = [(2, True, "r"), (2, False, "f"), (3, True, "r"), (3, False, "r"), (4, True, "t"), (4, False, "r"), (5, True, "r"), (5, False, "f"),
         (6, True, "r"), (6, False, "t"), (7, True, "f"), (7, False, "r"), (8, True, "r"), (8, False, "d"), (9, True, "n"), (9, False, "r"),
         (10, True, "r"), (11, False, "r"), (12, True, "r"), (12, False, "r")]


@pytest.mark.parametrize("case", range(len(EXACT)))
def test_exact_is_bit_equal(ctx, case):
    M, closed, rk = EXACT[case]
    m = M if closed else M - 1
    for kind in ("e", "h"):
        d = euclid(m, 300 + case) if kind == "e" else hops(m, 300 + case, 4)
        b, a, fx = rules_of(rk, m, 40 + case, closed)
        want = S.seam_tour_rules_exact(d, m, closed=closed, **kw_rules(b, a, fx))
        got = api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)
        assert got["cost_q"] == want["cost_q"]
        assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["dir"], want["dir"])
        again = api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)
        assert again["order"].tobytes() == got["order"].tobytes() and again["dir"].tobytes() == got["dir"].tobytes()
        assert api.seam_rules_check(got["order"], got["dir"], b, a, fx, closed=closed, ctx=ctx) == (0, 0)
        if M <= 7:
            assert got["cost_q"] == S.brute_force_rules(d, m, closed=closed, **kw_rules(b, a, fx))
        assert got["cost_q"] >= api.seam_tour_exact(ctx, d, closed)["cost_q"]   # rules never make a tour cheaper
        # the optimum is a local optimum of the search: started there, a descent ends after one pass
        back = api.seam_tour_rules(ctx, d, b, a, fx, closed=closed, order0=got["order"], dir0=got["dir"], n_starts=1)
        assert back["cost_q"] == got["cost_q"] and back["start_passes"].tolist() == [1]


def test_plan_batch_seam_rules():
    """examples/plan_batch.py --seams --seam-before --seam-fixed: the JSON gains seam_rules, and its tour keeps the rules"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "plan_batch.py"), "--grid", "32", "--points", "8", "--exact-paths", "--shortcut",
                        "--seams", "--seam-before", "1:2,3:1,1:2", "--seam-fixed", "2:1,0:0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sr = out["seam_rules"]
    assert (sr["before"], sr["after"], sr["fixed"], sr["n_prec"], sr["n_fixed"]) == ([1, 3, 1], [2, 1, 2], [1, 0, 2, 0], 2, 2)
    for tour in (sr["searched"], sr["exact"]):
        assert tour["order"][0] == 0 and sorted(tour["order"]) == [0, 1, 2, 3]
        assert api.seam_rules_check(tour["order"], tour["dir"], sr["before"], sr["after"], sr["fixed"], closed=True) == (0, 0)
    free = out["seams"]["searched"]
    broken = api.seam_rules_check(free["order"], free["dir"], sr["before"], sr["after"], sr["fixed"], closed=True)
    assert sr["unconstrained_breaks"] == dict(precedences=broken[0], directions=broken[1], cost=free["cost"])
    assert out["seams"]["exact"]["cost"] <= sr["exact"]["cost"] <= sr["searched"]["cost"]


def test_what_the_search_finds(ctx):
    """40 cases of 10 .. 15 seams: no searched tour is cheaper than the exact one and none breaks a rule (wa_gtsp_seam_rules_check).  In how
    many cases 1, 16 and 256 starts reach the optimum is printed, not asserted (profiles/seam_rules/README.md records it)."""
    hit = {1: 0, 16: 0, 256: 0}
    over = {1: 0.0, 16: 0.0, 256: 0.0}
    for case in range(40):
        m, closed = 10 + case % 6, bool(case & 1)
        d = euclid(m, 2000 + case)
        b, a, fx = S.random_rules(m, 2000 + case, closed)
        opt = api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)
        assert api.seam_rules_check(opt["order"], opt["dir"], b, a, fx, closed=closed, ctx=ctx) == (0, 0)
        for n in hit:
            r = api.seam_tour_rules(ctx, d, b, a, fx, closed=closed, n_starts=n, seed=case)
            assert r["cost_q"] >= opt["cost_q"]
            assert api.seam_rules_check(r["order"], r["dir"], b, a, fx, closed=closed, ctx=ctx) == (0, 0)
            hit[n] += r["cost_q"] == opt["cost_q"]
            over[n] += r["cost_q"] / opt["cost_q"] - 1
    print("seam rules, 40 cases of 10 .. 15 seams: optimum reached with 1 / 16 / 256 starts in %d / %d / %d cases; mean excess %.3f %% / %.3f %% / %.3f %%"
          % (hit[1], hit[16], hit[256], over[1] * 2.5, over[16] * 2.5, over[256] * 2.5))
