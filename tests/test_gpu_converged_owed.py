"""Owed evaporations (WA_CONVERGED_OWED): a window that commits whole in front of a generation that is enqueued in full whatever happens
-- a stamped one, or the last of a call -- also judges that generation; if every ant of it replays the path too the window is CARRIED, its flush is
the rows launch alone, and the sweep of the generation behind it multiplies every value W + 1 times while that generation's table blocks take the
path nodes' records from the commit's snapshot.

Every case is a three-way comparison, bit for bit, over the five trace arrays, the best cost and path, the ants of the last generation and the WHOLE
pheromone field: mechanism on == WA_CONVERGED_OWED=0 == the C oracle in DEV mode.  Every case that is there for the mechanism asserts from
wa_acs_converged_owed_info that the path it is there for was taken; with the switch off all counters are zero.

The searches are the 12^3 ones of test_gpu_converged_run.py, whose docstring lists the generations the oracle says are replays (every ant re-walks the
best path); the converged best path has 22 nodes.  What the cases expect is read off those lists:
  firm, stamped every 10th generation, one call: windows 31-39 (cut at 34), 41-49, 51-59, ..., 81-89 of nine generations and 91-98 of eight in front
      of the last generation; the stamped generations from 50 on and generation 99 are replays: five sweeps of 10 multiplications (in place) and one
      of 9 (out of place).  Every 5th: windows of four (5 multiplications, out of place) and 96-98 of three (4, in place).
  partial (rho 0.9), calls of 70, 4 and 26 generations: the first call ends with window 64-68 and generation 69, a replay (carried); the second is
      window 70-72 and generation 73, in which an ant leaves the path (whole, not carried: flushed as ever).
  partial, stamped every 4th: windows 65-67, 69-71, 77-79, 81-83 and 89-91 are carried; 73-75 commits nothing, 85-87 one generation, 93-95 two.
A window looks at the straggler pools and does nothing while ants are pending there; where that could hide a window the hand-over (which changes no
result) is switched off."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_converged_run as R
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)

pytestmark = pytest.mark.gpu

EXTRA = ("WA_CONVERGED_OWED", "WA_CONVERGED_READBACK")
NONE = dict(carried=0, merged=0, fallback=0, out_of_place=0, in_place=0)
PIECES = [1, 2, 7, 3, 11, 1, 1, 20, 5]


@contextlib.contextmanager
def switches(env):
    """the switches R.gpu does not know (it restores its own three): set for the solver's creation, put back afterwards"""
    old = {k: os.environ.get(k) for k in EXTRA}
    try:
        for k in EXTRA:
            os.environ.pop(k, None)
            if k in env:
                os.environ[k] = str(env[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run(ctx, dgrids, case, env, pieces=None, between=None, **kw):
    """R.gpu with the owed counters: (results per slot, wa_acs_converged_info per slot, wa_acs_converged_owed_info behind the last call).  The pieces
    are completed to the whole search, so that the counters are read behind its last generation."""
    gens = R.CASES[case][4]
    pieces = list(pieces or [gens])
    if sum(pieces) < gens:
        pieces.append(gens - sum(pieces))
    seen = {}

    def tap(s, done):
        seen.clear()
        seen.update(s.converged_owed_info())   # (host counters: no wait)
        if between:
            between(s, done)
    with switches(env):
        out, info = R.gpu(ctx, dgrids, case, {k: v for k, v in env.items() if k not in EXTRA}, pieces=pieces, between=tap, **kw)
    return out, info, dict(seen)


def three_way(ctx, dgrids, case, env, tag, **kw):
    """mechanism on == WA_CONVERGED_OWED=0 == oracle; returns (wa_acs_converged_info per slot, the owed counters) of the run with the mechanism on"""
    on, info, owed = run(ctx, dgrids, case, env, **kw)
    off, info_off, owed_off = run(ctx, dgrids, case, dict(env, WA_CONVERGED_OWED=0), **kw)
    print(tag, info, owed)
    for q in range(len(on)):
        want = R.ref(case, q)
        R.same(off[q], want, (tag, "owed off", q))
        R.same(on[q], want, (tag, "owed on", q))
        R.same(on[q], off[q], (tag, "on == off", q))
    assert info == info_off, (tag, info, info_off)            # what the windows commit does not depend on who pays the evaporations
    assert owed_off == NONE, (tag, owed_off)
    assert owed["merged"] == owed["carried"] == owed["out_of_place"] + owed["in_place"], (tag, owed)   # every carried window is paid for, once
    return info, owed


@pytest.mark.parametrize("period", [10, 5])
def test_stamped_generations_pay(ctx, dgrids, period):
    """windows of nine and of four generations between stamped ones: 10 multiplications in place, 5 out of place (and the window in front of the
    search's last generation, one generation shorter, the other way round)"""
    info, owed = three_way(ctx, dgrids, "firm", {}, ("stamped", period), profile=period)
    assert info[0]["whole"] > 0 and owed["merged"] > 0, (info, owed)
    if period == 10:
        assert owed["in_place"] >= 5 and owed["out_of_place"] >= 1, owed      # 50, 60, 70, 80, 90; 99
    else:
        assert owed["out_of_place"] >= 5 and owed["in_place"] >= 1, owed      # 45, 50, 55, ...; 99 behind window 96-98


@pytest.mark.parametrize("window", [3, 5])
def test_short_windows_and_uneven_calls(ctx, dgrids, window):
    """windows of 3 and 5 chained between stamped generations (only the last of a chain has a full generation behind it), calls of every length: a
    merged generation that is the last of its call, a call that begins right behind one"""
    info, owed = three_way(ctx, dgrids, "firm", dict(WA_CONVERGED_WINDOW=window), ("pieces", window), profile=10, pieces=PIECES)
    assert info[0]["whole"] > 0 and owed["merged"] > 0, (info, owed)


def test_whole_but_not_carried(ctx, dgrids):
    """rho 0.9, calls of 70, 4 and 26 generations: window 64-68 is carried into generation 69; window 70-72 commits whole and an ant leaves the path
    in generation 73: today's flush, sweep included"""
    info, owed = three_way(ctx, dgrids, "partial", {}, "partial 70 4 26", pieces=[70, 4, 26], stragglers=0)
    assert owed["fallback"] >= 1 and owed["merged"] >= 1, (info, owed)


def test_cut_windows_between_carried_ones(ctx, dgrids):
    """rho 0.9, stamped every 4th generation: windows of three; 73-75 commits nothing, 85-87 one generation, 93-95 two, five others are carried"""
    info, owed = three_way(ctx, dgrids, "partial", {}, "partial period 4", profile=4, stragglers=0)
    assert info[0]["cut"] > 0 and owed["carried"] >= 5, (info, owed)


def test_an_improvement_is_not_hidden(ctx, dgrids):
    """generation 31 is committed, generation 33 finds a better path (windows of one generation, a call of 33 generations first, as in
    test_gpu_converged_run.py); and the same search with stamped generations and the default window"""
    info, owed = three_way(ctx, dgrids, "improves", dict(WA_CONVERGED_WINDOW=1), "improves", pieces=[33], stragglers=0)
    best = R.ref("improves")["bestL"].view(np.float32)
    assert info[0]["generations"] > 0 and best[-1] < best[32], (info, best[32], best[-1])
    three_way(ctx, dgrids, "improves", {}, "improves, stamped", profile=4, pieces=[33], stragglers=0)


@pytest.mark.parametrize("kw", [dict(P=3, groups=1), dict(P=3, groups=2), dict(env=dict(WA_CONVERGED_READBACK=0))], ids=["batch", "groups", "no read-back"])
def test_paths_the_host_does_not_read(ctx, dgrids, kw):
    """batches, pipelined groups and WA_CONVERGED_READBACK=0: nothing is judged, nothing owed, results equal"""
    kw = dict(kw)
    env = kw.pop("env", {})
    on, info, owed = run(ctx, dgrids, "firm", env, profile=10, **kw)
    for q in range(len(on)):
        R.same(on[q], R.ref("firm", q), ("unread", sorted(kw.items()), q))
    assert all(i["generations"] > 0 for i in info), info
    assert owed == NONE, owed


@pytest.mark.parametrize("case", ["wide", "small"])
def test_colony_against_the_checking_lanes(ctx, dgrids, case):
    """the extra check pass with 64 ants and with 20"""
    info, owed = three_way(ctx, dgrids, case, {}, ("colony", case), profile=5)
    assert owed["merged"] > 0, (info, owed)


@functools.lru_cache(maxsize=None)
def field_after(case, gens):
    """the oracle's field behind `gens` generations of the search"""
    n, occ, colony, rho, _, seed = R.CASES[case]
    g, (sid, eid) = R.ogrid(n, occ)
    a = O.Acs(g)
    a.solve(sid, eid, gens, float(colony / 0.35), fixed_colony=colony, mode=O.DEV, seed=seed, stream=0, rho=rho)
    return R.bits(a.pheromone())


def test_a_read_behind_a_merged_generation(ctx, dgrids):
    """firm, stamped every 10th generation, calls of 51, 9 and 40: the second call is window 51-58 and generation 59, which pays the window's eight
    evaporations with its own.  sync() and pheromone() directly behind it, then on"""
    merged, fields = {}, {}

    def between(s, done):
        merged[done] = s.converged_owed_info()["merged"]
        if done == 60:
            s.sync()
            fields[done] = R.bits(s.pheromone(0))
    on, info, owed = run(ctx, dgrids, "firm", {}, pieces=[51, 9, 40], profile=10, between=between)
    R.same(on[0], R.ref("firm"), "read in between")
    assert merged[60] == merged[51] + 1, merged               # the only full generation of the second call is generation 59
    assert np.array_equal(fields[60], field_after("firm", 60))
    assert owed["merged"] > merged[60], (owed, merged)        # ... and on: 60 is stamped, windows 61-69, ... follow
