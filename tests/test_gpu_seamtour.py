"""wa_gtsp_seam_tour / wa_gtsp_seam_tour_exact on the device against the numpy restatement (tests/seamtour_ref.py), byte for byte: order, direction,
cost, every start's cost and passes, the summary.  Seeded Euclidean endpoint sets and small-integer matrices (equal-cost ties)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import seamtour_ref as R
from welding_robot_amd import _lib as L
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
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


def given_start(m, seed):
    rs = np.random.RandomState(seed)
    return rs.permutation(m).astype(np.int32), rs.randint(0, 2, m).astype(np.uint8)


def same(got, want):
    assert np.array_equal(got["order"], want["order"]) and got["order"].dtype == np.int32
    assert np.array_equal(got["dir"], want["dir"]) and got["dir"].dtype == np.uint8
    assert got["cost_q"] == want["cost_q"]
    assert np.array_equal(got["start_cost_q"], want["start_cost_q"])
    assert np.array_equal(got["start_passes"], want["start_passes"])
    assert got["summary"] == want["summary"]


# (kind, m, scale / hi, closed, or_len, n_starts, given start): M = m or m + 1 runs from 1 to 201; 64 / 65 is where a descent goes from a
# wavefront to a workgroup, 100 / 101 where a narrow W stops fitting LDS; scale 1e4 gives costs above 2^32 quanta (W stays 64-bit)
CASES = [
    ("e", 1, 1, True, 3, 3, False), ("e", 1, 1, False, 3, 3, True), ("e", 2, 1, True, 3, 4, False), ("e", 2, 1, False, 2, 4, True),
    ("e", 3, 1, True, 3, 5, False), ("h", 3, 4, False, 1, 5, False), ("e", 4, 1, True, 0, 6, True), ("h", 5, 3, True, 3, 16, False),
    ("e", 7, 1, False, 3, 9, True), ("h", 8, 2, True, 2, 32, False), ("e", 12, 1, True, 3, 33, False), ("h", 12, 6, False, 3, 20, True),
    ("e", 16, 1e4, True, 3, 7, False), ("e", 20, 1, False, 1, 12, False), ("h", 24, 3, True, 3, 10, True), ("e", 32, 1, True, 3, 70, False),
    ("e", 32, 1, False, 3, 40, True), ("h", 32, 6, False, 0, 8, False), ("e", 33, 1, True, 2, 5, False), ("e", 40, 1e4, False, 3, 6, True),
    ("h", 48, 4, True, 3, 6, False), ("e", 63, 1, False, 3, 5, False), ("e", 64, 1, True, 3, 9, True), ("e", 64, 1e4, True, 1, 5, False),
    ("e", 64, 1, False, 3, 4, False), ("h", 65, 5, True, 3, 3, True), ("e", 70, 1e4, True, 2, 3, False), ("e", 80, 1, False, 3, 3, False),
    ("h", 90, 3, True, 0, 4, True), ("e", 99, 1, False, 3, 2, False), ("e", 100, 1, True, 3, 3, False), ("e", 100, 1, False, 1, 2, True),
    ("h", 101, 6, True, 3, 2, False), ("e", 120, 1, True, 3, 3, True), ("e", 128, 1e4, False, 3, 2, False), ("h", 150, 4, False, 2, 2, False),
    ("e", 160, 1, True, 3, 2, False), ("e", 200, 1, True, 3, 2, True), ("e", 200, 1, False, 3, 2, False), ("h", 200, 2, True, 3, 2, False),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_search_is_bit_equal_to_the_restatement(ctx, case):
    kind, m, par, closed, or_len, n_starts, given = CASES[case]
    d = euclid(m, 100 + case, par) if kind == "e" else hops(m, 100 + case, par)
    o0, d0 = given_start(m, case) if given else (None, None)
    kw = dict(closed=closed, or_len=or_len, n_starts=n_starts, seed=0xC0FFEE + case, order0=o0, dir0=d0)
    want = R.seam_tour(d, m, **kw)
    got = api.seam_tour(ctx, d, **kw)
    same(got, want)
    assert want["summary"]["n_capped"] == 0
    assert got["cost_q"] <= got["summary"]["start0_cost_q_out"] <= got["summary"]["start0_cost_q_in"]
    again = api.seam_tour(ctx, d, **kw)   # the same bytes on every call
    for k in ("order", "dir", "start_cost_q", "start_passes"):
        assert got[k].tobytes() == again[k].tobytes()
    assert got["summary"] == again["summary"]


@pytest.mark.parametrize("m,closed", [(24, True), (70, False)])
def test_max_passes_that_binds(ctx, m, closed):
    d = euclid(m, 7 + m)
    kw = dict(closed=closed, or_len=3, n_starts=5, seed=99)
    free = R.seam_tour(d, m, **kw)
    cap = int(free["start_passes"].min()) - 1   # below what every start takes on its own: every start is cut short
    assert cap >= 2
    want = R.seam_tour(d, m, max_passes=cap, **kw)
    assert want["summary"]["n_capped"] == 5 and want["start_passes"].tolist() == [cap] * 5
    same(api.seam_tour(ctx, d, max_passes=cap, **kw), want)
    # ... and a cap that only some starts reach
    cap = int(np.sort(free["start_passes"])[2])
    want = R.seam_tour(d, m, max_passes=cap, **kw)
    assert 0 < want["summary"]["n_capped"] < 5
    same(api.seam_tour(ctx, d, max_passes=cap, **kw), want)


@pytest.mark.parametrize("M", range(1, 17))
def test_exact_is_bit_equal(ctx, M):
    for closed in (True, False):
        m = M if closed else M - 1
        if m < 1:
            continue
        for kind in ("e", "h"):
            d = euclid(m, 300 + M) if kind == "e" else hops(m, 300 + M, 4)
            want = R.seam_tour_exact(d, m, closed)
            got = api.seam_tour_exact(ctx, d, closed)
            assert got["cost_q"] == want["cost_q"]
            assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["dir"], want["dir"])
            assert api.seam_tour_exact(ctx, d, closed)["order"].tobytes() == got["order"].tobytes()
            if M <= 7:
                assert got["cost_q"] == R.brute_force(d, m, closed)
            s = api.seam_tour(ctx, d, closed=closed, n_starts=16, seed=M)
            assert got["cost_q"] <= s["start_cost_q"].min()
            back = api.seam_tour(ctx, d, closed=closed, order0=got["order"], dir0=got["dir"], n_starts=1)
            assert back["cost_q"] == got["cost_q"] and back["start_passes"].tolist() == [1]


def test_refused_calls_leave_the_outputs_untouched(ctx):
    lib = ctx.lib
    m = 6
    good = euclid(m, 1)

    def call(dist=good, m=m, closed=1, or_len=3, n_starts=4, max_passes=100, order0=None, dir0=None, null=()):
        dist = np.ascontiguousarray(dist, np.float64)
        p = L.SeamParams(closed, or_len, n_starts, max_passes, 5)
        order, dirs = np.full(16, -7, np.int32), np.full(16, 9, np.uint8)
        costs, passes = np.full(8, -7, np.int64), np.full(8, -7, np.int32)
        s = L.SeamSummary()
        C.memset(C.byref(s), 0x5a, C.sizeof(s))
        before = bytes(s)
        ptr = lambda name, a: None if name in null else a.ctypes.data
        o0 = None if order0 is None else np.asarray(order0, np.int32)
        d0 = None if dir0 is None else np.asarray(dir0, np.uint8)
        rc = lib.wa_gtsp_seam_tour(ctx.h, ptr("dist", dist), m, None if "params" in null else C.byref(p), api._ptr(o0), api._ptr(d0),
                              ptr("order", order), ptr("dir", dirs), costs.ctypes.data, passes.ctypes.data,
                              None if "sum" in null else C.byref(s))
        untouched = (order == -7).all() and (dirs == 9).all() and (costs == -7).all() and (passes == -7).all() and bytes(s) == before
        return rc, untouched

    assert call()[0] == 0
    bad = []
    for name in ("dist", "params", "order", "dir", "sum"):
        bad.append(call(null=(name,)))
    bad += [call(m=0), call(m=1025, dist=np.zeros((2, 2))), call(or_len=-1), call(or_len=4), call(n_starts=0), call(n_starts=(1 << 20) + 1),
            call(max_passes=0), call(max_passes=(1 << 20) + 1), call(order0=[0, 1, 2, 3, 4, 4]), call(order0=[0, 1, 2, 3, 4, 6]),
            call(order0=[-1, 1, 2, 3, 4, 5]), call(dir0=[0, 1, 0, 1, 0, 2])]
    for v in (-1e-9, np.nan, np.inf, float(1 << 20), 1e300):
        e = good.copy()
        e[3, 8] = v
        bad.append(call(dist=e))
    for rc, untouched in bad:
        assert rc == ARG and untouched
    e = good.copy()   # what is never read may hold anything
    e[8, 3], e[4, 4], e[4, 5] = np.nan, -1, np.inf
    assert call(dist=e)[0] == 0
    assert lib.wa_gtsp_seam_tour(None, None, 0, None, None, None, None, None, None, None, None) == ARG

    def exact(dist, m, closed=1, null=()):
        dist = np.ascontiguousarray(dist, np.float64)
        order, dirs, cost = np.full(32, -7, np.int32), np.full(32, 9, np.uint8), np.full(1, -7, np.int64)
        ptr = lambda name, a: None if name in null else a.ctypes.data
        rc = lib.wa_gtsp_seam_tour_exact(ctx.h, ptr("dist", dist), m, closed, ptr("order", order), ptr("dir", dirs), ptr("cost", cost))
        return rc, (order == -7).all() and (dirs == 9).all() and (cost == -7).all()

    assert exact(good, m)[0] == 0
    for name in ("dist", "order", "dir", "cost"):
        assert exact(good, m, null=(name,)) == (ARG, True)
    assert exact(good, 0) == (ARG, True)
    assert exact(euclid(17, 2), 17) == (CAPACITY, True)
    assert exact(euclid(16, 2), 16, closed=0) == (CAPACITY, True)
    assert exact(euclid(16, 2), 16)[0] == 0 and exact(euclid(15, 2), 15, closed=0)[0] == 0
    e = good.copy()
    e[0, 2] = -1
    assert exact(e, m) == (ARG, True)


def test_c5_seams_from_the_acs_tsp_start(ctx):
    """C5's geometry (256^3 synthetic grid, 64 weld points) as 32 seams: points 2k and 2k+1 form seam k.  The golden file holds the rows
    of 4 of the 64 sources only, so the whole hop matrix comes from the device (those 4 rows are checked on the way).  Start 0 is the
    seam-level ACS-TSP tour on D[s][t] = the cheapest of the four end combinations, each seam entered so that the hop to the next one is
    the cheaper; a descent never raises the cost, so the searched tour costs at most that start: no margin."""
    gold = json.load(open(os.path.join(GOLD, "geodesic_c5_rows.json")))
    n = 256
    free = synth.synth_grid(n)[0]
    pts = synth.synth_weld_points(free, n, 64)
    ax = np.arange(n, dtype=np.float32)
    g = api.Grid.from_occupancy(ctx, free, ax, ax, ax, 1.0, 0)
    hop = g.geodesic_matrix(pts)
    g.close()
    assert np.array_equal(hop[gold["sources"]], np.array(gold["rows"], np.int32)) and (hop >= 0).all()
    d = hop.astype(np.float64)
    m = 32
    D = d.reshape(m, 2, m, 2).min(axis=(1, 3))
    np.fill_diagonal(D, 0)
    t = api.gtsp_solve(ctx, D, seed=7)
    order0 = [int(e[0]) for e in t["edges"][0]]
    assert sorted(order0) == list(range(m))
    dir0 = [int(d[2 * s:2 * s + 2, 2 * u:2 * u + 2].min(axis=1).argmin() == 0) for s, u in zip(order0, order0[1:] + order0[:1])]
    for closed in (True, False):
        kw = dict(closed=closed, or_len=3, n_starts=256, seed=11, order0=order0, dir0=dir0)
        r = api.seam_tour(ctx, d, **kw)
        s = r["summary"]
        print("C5 seams closed=%d: ACS-TSP start %d, its descent %d, searched %d (hops; start %d of %d, %d passes)"
              % (closed, s["start0_cost_q_in"] >> 20, s["start0_cost_q_out"] >> 20, s["cost_q"] >> 20, s["best_start"], s["n_starts"],
                 s["passes_total"]))
        assert s["cost_q"] <= s["start0_cost_q_out"] <= s["start0_cost_q_in"]
        assert s["cost_q"] % R.Q == 0 and s["n_capped"] == 0
        want = R.seam_tour(d, m, **dict(kw, n_starts=3))
        assert want["start_cost_q"].tolist() == r["start_cost_q"][:3].tolist()
        assert want["summary"]["start0_cost_q_in"] == s["start0_cost_q_in"]
