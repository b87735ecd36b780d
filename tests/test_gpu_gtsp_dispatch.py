"""Seam ordering (wa_gtsp_solve) on every kernel the solver can dispatch, against the C oracle (oracle_lib.gtsp_solve,
pinned to the reference by tests/test_oracle_vs_ref.py): each variant at its size boundaries, the default dispatch of
batches, and degenerate distance matrices (coincident cities, ties, distances above the INF sentinel, scales that
overflow or underflow the pheromone / heuristic products, cnt of 0 and 1).

Every comparison is exact: the iteration count, the cost bits, the tour edges and the pheromone bits.  The only
allowance is the payload of a NaN (IEEE 754 leaves it open, and x86 and gfx950 produce different default NaNs):
NaN must meet NaN at the same places."""
import numpy as np
import pytest

import oracle_lib as O
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

INF = float(0x3f3f3f3f)   # ACS_GTSP.hpp:19, the "no tour yet" cost


# ------------------------------------------------------------------ the dispatch rule
# Mirrors welding_robot_amd/csrc/host_gtsp.inc, wa_gtsp_solve: `nw`, `in_lds` and `wave_path` (the block opening with
# "fast path: lanes = ants"), `nc` / `stage` of the wave branch, and the three-way
# `if (n <= 256 && wave_path && !GENERIC) ... else if (n <= 256 && !GENERIC) ... else k_gtsp` below them.
def dispatch(n, n_instances=1, wave=None, generic=False):
    """name of the construct kernel wa_gtsp_solve launches; wave / generic: the WA_GTSP_WAVE / WA_GTSP_GENERIC knobs"""
    if generic or n > 256:
        return "k_gtsp"
    wave_path = n_instances * n <= 1024 if wave is None else wave
    if wave_path:
        return "k_gtspw_construct<8, true>" if n <= 128 else "k_gtspw_construct<16, false>"   # stage: 8*n*n <= 128 KiB
    nw = 1 if n <= 64 else (2 if n <= 128 else 4)
    in_lds = 8 * (64 * nw + 1) * n <= 140 * 1024                                               # always true for nw = 2
    return {1: "k_gtsp_fast<1, true, true>", 2: "k_gtsp_fast<2, %s, false>" % ("true" if in_lds else "false"),
            4: "k_gtsp_fast<4, false, false>"}[nw]


# variant -> (knobs, seam counts at its boundaries).  Every kernel the rule can reach is here; k_gtsp_fast<2, false,
# false> cannot be reached (65..128 cities always fit in LDS), see test_dispatch_table.
VARIANTS = {
    "wave8": (dict(wave=True), (2, 3, 63, 64, 65, 127, 128)),
    "wave16": (dict(wave=True), (129, 255, 256)),
    "fast1": (dict(wave=False), (2, 3, 63, 64)),
    "fast2": (dict(wave=False), (65, 127, 128)),
    "fast4": (dict(wave=False), (129, 255, 256)),
    "generic_forced": (dict(generic=True), (2, 3, 63, 64, 65, 128, 129, 255, 256)),
    "generic": (dict(), (257, 300, 400)),
}
KERNEL = {"wave8": "k_gtspw_construct<8, true>", "wave16": "k_gtspw_construct<16, false>",
          "fast1": "k_gtsp_fast<1, true, true>", "fast2": "k_gtsp_fast<2, true, false>",
          "fast4": "k_gtsp_fast<4, false, false>", "generic_forced": "k_gtsp", "generic": "k_gtsp"}


def cap(n):
    """iteration cap that keeps the oracle's run short (0 = run to the stagnation stop)"""
    return 0 if n <= 65 else (12 if n <= 128 else (4 if n <= 256 else 2))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture
def knobs(monkeypatch):
    """set the dispatch knobs of one variant (the library reads them on every call)"""
    def set_(wave=None, generic=False):
        monkeypatch.delenv("WA_GTSP_WAVE", raising=False)
        monkeypatch.delenv("WA_GTSP_GENERIC", raising=False)
        if wave is not None:
            monkeypatch.setenv("WA_GTSP_WAVE", "1" if wave else "0")
        if generic:
            monkeypatch.setenv("WA_GTSP_GENERIC", "1")
    set_()
    return set_


# ------------------------------------------------------------------ inputs
def points(rs, n):
    P = rs.uniform(0, 1, (n, 3))
    return np.abs(P[:, None, :] - P[None, :, :]).sum(-1)


def clusters(rs, n):
    """two clusters of coincident cities: zero distances inside, one distance between"""
    side = rs.uniform(size=n) < 0.5
    side[0], side[-1] = True, False
    return np.where(side[:, None] == side[None, :], 0.0, 1.375)


def ties(rs, n):
    """integer points, distances rounded to 3 decimals: many exactly equal distances and tours"""
    P = rs.randint(0, 4, (n, 3)).astype(np.float64)
    return np.round(np.abs(P[:, None, :] - P[None, :, :]).sum(-1) / 7.0, 3)


def asym(rs, n):
    d = rs.uniform(0.05, 1.0, (n, n))
    np.fill_diagonal(d, 0.0)
    return d


# name -> (matrix(rs, n), cnt or None = the default n*(n-1)/2, REF mode meaningful).  cnt = 0 on coincident cities makes
# pheromone_0 = 0/0 = NaN: no ant ever finds a city, and the reference then draws at every step, n*n draws per
# iteration instead of the n*(n-1) the kernels replay, so that case is compared in DEV mode only.
DEGENERATE = {
    "coincident": (lambda rs, n: np.zeros((n, n)), None, True),
    "coincident_cnt1": (lambda rs, n: np.zeros((n, n)), 1, True),
    "coincident_cnt0": (lambda rs, n: np.zeros((n, n)), 0, False),
    "clusters": (clusters, None, True),
    "ties": (ties, None, True),
    "asymmetric": (asym, None, True),
    "above_inf": (lambda rs, n: 2e9 + points(rs, n) * 1e9, None, True),   # every tour costs more than INF
    "scale_1e-200": (lambda rs, n: points(rs, n) * 1e-200, None, True),   # pheromone_0 ~ 1e200
    "scale_1e-300": (lambda rs, n: points(rs, n) * 1e-300, None, True),   # pheromone_0 * h^6 overflows to +inf
    "scale_1e150": (lambda rs, n: points(rs, n) * 1e150, None, True),     # h^6 underflows to 0
    "cnt0": (points, 0, True),                                            # pheromone_0 = 0
    "cnt1": (points, 1, True),
}


# ------------------------------------------------------------------ comparison
def f64_same(a, b):
    """bit-identical fp64 values, NaN payloads aside"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def is_permutation_tour(edges):
    """edges (r, s) of one closed tour visiting every city exactly once"""
    n = len(edges)
    return (sorted(edges[:, 0].tolist()) == list(range(n)) and np.array_equal(edges[1:, 0], edges[:-1, 1])
            and edges[-1, 1] == edges[0, 0])


def check(t, q, o, tag, pher=True):
    assert t["iters"][q] == o["iters"], (tag, t["iters"][q], o["iters"])
    assert f64_same(t["L"][q], o["L"]), (tag, t["L"][q], o["L"])
    assert np.array_equal(t["edges"][q], o["edges"]), tag
    if pher:
        assert f64_same(t["pher"][q], o["pher"]), tag
    if is_permutation_tour(o["edges"]):
        assert is_permutation_tour(t["edges"][q]), tag


def run_dev(ctx, d, cnt=None, mi=0, seed=5, stream=1):
    o = O.gtsp_solve(d, cnt=cnt, mode=O.DEV, seed=seed, stream=stream, max_iterations=mi, want_pher=True)
    t = api.gtsp_solve(ctx, d, cnt=cnt, mode=api.RNG_DEV, seed=seed, stream=stream, max_iterations=mi, want_pher=True)
    return t, o


def run_ref(ctx, d, cnt=None, mi=0, srand=77):
    """REF mode: one libc stream, seeded like the reference's srand(); the state afterwards must agree too"""
    rng = O.srand(srand)
    st = np.array(list(rng.r) + [rng.f, rng.b], np.int32)
    o = O.gtsp_solve(d, cnt=cnt, mode=O.REF, rng=rng, max_iterations=mi, want_pher=True)
    t = api.gtsp_solve(ctx, d, cnt=cnt, mode=api.RNG_REF, rand_state=st, max_iterations=mi, want_pher=True)
    return t, o, rng


def check_ref(t, o, rng, tag):
    check(t, 0, o, tag)
    assert [int(v) for v in t["rand_state"][:31]] == list(rng.r)[:31], tag
    assert (int(t["rand_state"][34]), int(t["rand_state"][35])) == (rng.f, rng.b), tag


# ------------------------------------------------------------------ tests
def test_dispatch_table():
    """the table above covers exactly the kernels the rule can reach"""
    reach = {dispatch(n, i, w, g) for n in range(2, 513) for i in (1, 8, 64) for w in (None, True, False)
             for g in (False, True)}
    assert reach == set(KERNEL.values())
    for name, (kn, sizes) in VARIANTS.items():
        for n in sizes:
            assert dispatch(n, 1, **kn) == KERNEL[name], (name, n)
    # the defaults of a single seam ordering and of the batches below
    assert dispatch(64) == KERNEL["wave8"] and dispatch(200) == KERNEL["wave16"] and dispatch(300) == KERNEL["generic"]
    assert dispatch(48, 24) == KERNEL["fast1"] and dispatch(100, 12) == KERNEL["fast2"]
    assert dispatch(200, 8) == KERNEL["fast4"] and dispatch(64, 4) == KERNEL["wave8"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_boundaries_dev(ctx, knobs, variant):
    kn, sizes = VARIANTS[variant]
    knobs(**kn)
    rs = np.random.RandomState(sum(map(ord, variant)))
    for n in sizes:
        d = points(rs, n)
        if n >= 9:
            d[3], d[:, 3] = d[5], d[:, 5]   # two coincident cities: a zero distance and tied rows
            d[3, 3] = d[5, 5] = 0.0
        t, o = run_dev(ctx, d, mi=cap(n), seed=1000 + n, stream=n)
        check(t, 0, o, (variant, n))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_boundaries_ref(ctx, knobs, variant):
    kn, sizes = VARIANTS[variant]
    knobs(**kn)
    rs = np.random.RandomState(7 + sum(map(ord, variant)))
    for n in sizes:
        t, o, rng = run_ref(ctx, points(rs, n), mi=min(cap(n) or 9, 9), srand=n)
        check_ref(t, o, rng, (variant, n))


# all cities at one point, at the seam counts of the issue that each variant can take (full runs up to 65 seams:
# the run stops on stagnation at n + 2 iterations; beyond, a cap)
COINCIDENT_N = (2, 3, 64, 65, 200, 300)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_coincident_cities(ctx, knobs, variant):
    kn, sizes = VARIANTS[variant]
    knobs(**kn)
    lo, hi = min(sizes), max(sizes)
    for n in [m for m in COINCIDENT_N if lo <= m <= hi]:
        d = np.zeros((n, n))
        for cnt in (None, 1, 0):
            mi = 0 if n <= 65 else 6
            t, o = run_dev(ctx, d, cnt=cnt, mi=mi, seed=9, stream=n)
            check(t, 0, o, (variant, n, cnt))
            if cnt is None:
                assert o["L"] == 0.0 and np.all(np.isposinf(o["pher"]))
                assert np.array_equal(o["edges"][:, 0], np.arange(n))     # 0 -> 1 -> ... -> n-1 -> 0
                assert mi or o["iters"] == n + 2
        if lo <= n <= 65:
            t, o, rng = run_ref(ctx, d, srand=n)
            check_ref(t, o, rng, (variant, n, "ref"))


# one seam count per variant for the degenerate matrices (full runs up to 65 seams, three iterations beyond)
DEGENERATE_N = {"wave8": 65, "wave16": 129, "fast1": 64, "fast2": 65, "fast4": 129, "generic_forced": 40, "generic": 257}


@pytest.mark.parametrize("case", list(DEGENERATE))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_degenerate_matrices(ctx, knobs, variant, case):
    kn, _ = VARIANTS[variant]
    knobs(**kn)
    make, cnt, ref_ok = DEGENERATE[case]
    rs = np.random.RandomState(sum(map(ord, case)))
    n = DEGENERATE_N[variant]
    d = make(rs, n)
    mi = 0 if n <= 65 else 3
    t, o = run_dev(ctx, d, cnt=cnt, mi=mi, seed=3, stream=2)
    check(t, 0, o, (variant, case, n))
    if case == "above_inf":   # no tour ever improves: no edges, the INF cost, stop after n + 1 iterations
        assert o["L"] == INF and not o["edges"].any() and (mi or o["iters"] == n + 1)
    if ref_ok:
        t, o, rng = run_ref(ctx, d, cnt=cnt, mi=mi or 12, srand=n)
        check_ref(t, o, rng, (variant, case, n, "ref"))


# ------------------------------------------------------------------ batches: the default dispatch, no knob
def _batch(ctx, mats, mi, stream0=40, seed=17, cnt=None):
    d = np.stack(mats)
    t = api.gtsp_solve(ctx, d, cnt=cnt, mode=api.RNG_DEV, seed=seed, stream=stream0, max_iterations=mi, want_pher=True)
    out = []
    for q in range(len(mats)):
        o = O.gtsp_solve(d[q], cnt=cnt, mode=O.DEV, seed=seed, stream=stream0 + q, max_iterations=mi, want_pher=True)
        check(t, q, o, (len(mats), d.shape[1], q))
        out.append(o)
    return out


@pytest.mark.parametrize("n_inst,n,mi", [(24, 48, 0), (12, 100, 10), (8, 200, 4), (3, 300, 2), (5, 200, 4)])
def test_default_batch(ctx, knobs, n_inst, n, mi):
    """24 x 48 -> k_gtsp_fast<1>, 12 x 100 -> <2>, 8 x 200 -> <4>, 3 x 300 -> k_gtsp, 5 x 200 -> the wave kernel"""
    knobs()
    rs = np.random.RandomState(n_inst * 1000 + n)
    makers = (points, ties, asym, clusters)
    _batch(ctx, [makers[q % len(makers)](rs, n) for q in range(n_inst)], mi)


@pytest.mark.parametrize("n_inst,n,kn", [(24, 48, dict()), (4, 64, dict()), (6, 40, dict(generic=True))])
def test_batch_with_an_early_stop(ctx, knobs, n_inst, n, kn):
    """the stagnation stop is per instance: coincident cities stop at n + 2 iterations, their neighbours run on
    (lanes-as-ants, wave and generic kernels)"""
    knobs(**kn)
    rs = np.random.RandomState(n)
    mats = [points(rs, n) for _ in range(n_inst)]
    mats[1] = np.zeros((n, n))
    mats[-1] = 2e9 + mats[-1]   # never improves: stops at n + 1
    o = _batch(ctx, mats, 0)
    assert o[1]["iters"] == n + 2 and o[-1]["iters"] == n + 1
    assert max(x["iters"] for x in o) > n + 2
