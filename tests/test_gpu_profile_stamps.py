"""Stamps of wa_acs_profile (csrc/host_acs.inc): event pairs come from a pool that wa_acs_sync refills, and on the fused DEV path the walk launch and
apply + table carry their start/stop events themselves, as the sweep-carrying launch does (WA_PROF_DISPATCH=0: the recorded pairs).

Stamping changes no result: every search here is held bit for bit -- the five trace arrays, the best cost and path, the ants of the last generation and
the whole pheromone field -- against the same search with profiling off and against the C oracle in DEV mode (the REF-mode solver against the oracle's
REF mode), through the harness of test_gpu_converged_run.py and its 12^3 search `firm`.  The launch counts expected per class:
  fused path (DEV mode; dense, lazy, 26 neighbours): one walk, one sweep-carrying and one apply + table launch per stamped generation and group, no
      rank launch;
  plain path (REF mode): one pair per class and stamped generation, the rank launch included.
A generation g of a search is stamped when g is a multiple of the period, so a run of G generations has ceil(G / period) of them."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_converged_run as R
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

KEYS = ("WA_PROF_DISPATCH", "WA_CONVERGED_RUN", "WA_CONVERGED_WINDOW", "WA_CONVERGED_NODES")
N, OCC, COLONY, RHO, _, SEED = R.CASES["firm"]


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
            if k in env:
                os.environ[k] = str(env[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def want(gens, stream=0, nb=6):
    """the oracle's run of `firm` over `gens` generations (R.ref for its own 100), computed once and never modified"""
    if gens == R.CASES["firm"][4]:
        return R.ref("firm", stream, nb)
    g, (sid, eid) = R.ogrid(N, OCC)
    a = O.Acs(g, nb=nb)
    tr = a.solve(sid, eid, gens, float(COLONY / 0.35), fixed_colony=COLONY, mode=O.DEV, seed=SEED, stream=stream, rho=RHO)
    lens, L = a.last_ants()
    return dict(steps=tr["steps"], finite=tr["finite"], colony=tr["colony"], bestL=R.bits(tr["bestL"]), iterbestL=R.bits(tr["iterbestL"]),
                cost=R.bits(a.best_L), path=a.best_path()[0], field=R.bits(a.pheromone()), antL=R.bits(L), antLen=lens)


def solver(ctx, dgrids, env, gens, P=1, groups=1, nb=6, lazy=False):
    """a solver created under the switches in `env`, with `firm` begun on P streams"""
    _, (sid, eid) = R.ogrid(N, OCC)
    with switches(env):
        s = api.AcsSolver(ctx, dgrids(N, OCC), n_slots=P, max_colony=COLONY, neighbourhood=nb, lazy=lazy)
    s.set_pipeline(groups)
    p = api.default_params(max_iteration=gens, predict=float(COLONY / 0.35), fixed_colony=COLONY, rng_mode=api.RNG_DEV, seed=SEED, rho=RHO)
    s.begin(p, [sid] * P, [eid] * P, streams=list(range(P)))
    return s


def stamped_run(ctx, dgrids, env, period, gens=100, pieces=None, **kw):
    """(results per slot, profile_read) of `firm` stamped every period-th generation (0: profiling off)"""
    s = solver(ctx, dgrids, env, gens, **kw)
    if period:
        s.profile(True, period)
    for c in (pieces or [gens]):
        s.run(c)
    pr = s.profile_read()
    out = [R.collect(s, q, gens) for q in range(kw.get("P", 1))]
    s.close()
    return out, pr


def stamps_of(gens, period):
    return (gens + period - 1) // period


@pytest.mark.parametrize("dispatch", [1, 0])
@pytest.mark.parametrize("period", [1, 3, 10])
def test_periods_change_no_result(ctx, dgrids, period, dispatch):
    """periods 1, 3 and 10, with per-dispatch stamps and with the recorded pairs: results equal to profiling off and to the oracle; three launches per
    stamped generation on the fused path"""
    env = dict(WA_PROF_DISPATCH=dispatch)
    on, pr = stamped_run(ctx, dgrids, env, period)
    off, pr_off = stamped_run(ctx, dgrids, env, 0)
    R.same(off[0], want(100), ("off", period, dispatch))
    R.same(on[0], want(100), ("on", period, dispatch))
    n = stamps_of(100, period)
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=n, rank=0, evaporate=n, deposit=n), pr
    assert all(pr[k]["ms"] > 0 for k in ("walk", "evaporate", "deposit")), pr
    assert all(v["launches"] == 0 and v["ms"] == 0 for v in pr_off.values()), pr_off


@pytest.mark.parametrize("dispatch", [1, 0])
@pytest.mark.parametrize("kind", ["lazy", "nb26", "batch"])
def test_launch_counts_of_the_other_fused_solvers(ctx, dgrids, kind, dispatch):
    """lazily evaporating, 26 neighbours, and a batch of two searches in two pipelined groups (each group stamps its own launches)"""
    kw = dict(lazy=dict(lazy=True), nb26=dict(nb=26), batch=dict(P=2, groups=2))[kind]
    on, pr = stamped_run(ctx, dgrids, dict(WA_PROF_DISPATCH=dispatch), 3, **kw)
    for q in range(len(on)):
        R.same(on[q], want(100, q, kw.get("nb", 6)), (kind, dispatch, q))
    n = stamps_of(100, 3) * kw.get("groups", 1)
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=n, rank=0, evaporate=n, deposit=n), pr
    assert all(pr[k]["ms"] > 0 for k in ("walk", "evaporate", "deposit")), pr


@pytest.mark.parametrize("dispatch", [1, 0])
def test_ref_mode_keeps_the_recorded_pairs(ctx, dgrids, dispatch):
    """REF mode runs the plain path: walk (several launches where it speculates), rank, sweep, deposit -- one stamp per class and stamped generation"""
    gens = 40
    g, (sid, eid) = R.ogrid(N, OCC)
    with switches(dict(WA_PROF_DISPATCH=dispatch)):
        s = api.AcsSolver(ctx, dgrids(N, OCC), n_slots=1, max_colony=COLONY)
    s.srand(SEED)
    s.begin(api.default_params(max_iteration=gens, predict=float(COLONY / 0.35), fixed_colony=COLONY, rng_mode=api.RNG_REF, rho=RHO), [sid], [eid])
    s.profile(True, 3)
    s.run(gens)
    pr = s.profile_read()
    t = s.trace(0)
    s.close()
    a = O.Acs(g)
    tr = a.solve(sid, eid, gens, float(COLONY / 0.35), fixed_colony=COLONY, mode=O.REF, rng=O.srand(SEED), rho=RHO)
    assert np.array_equal(R.bits(t["bestL"][:gens]), R.bits(tr["bestL"])) and np.array_equal(t["steps"][:gens], tr["steps"])
    n = stamps_of(gens, 3)
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=n, rank=n, evaporate=n, deposit=n), pr
    assert all(v["ms"] > 0 for v in pr.values()), pr


def test_300_stamped_generations_and_one_read(ctx, dgrids):
    """every generation stamped, nothing read until the end: 900 pairs outstanding, all harvested by the one read"""
    on, pr = stamped_run(ctx, dgrids, {}, 1, gens=300, pieces=[50] * 6)
    R.same(on[0], want(300), "300")
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=300, rank=0, evaporate=300, deposit=300), pr
    assert all(pr[k]["ms"] > 0 for k in ("walk", "evaporate", "deposit")), pr


def test_fifty_rounds_reuse_the_pool(ctx, dgrids):
    """enable, run(3), read, fifty times on one solver: from the second round on every pair comes out of the pool; each read reports its own round"""
    s = solver(ctx, dgrids, {}, 150)
    for r in range(50):
        s.profile(True, 1)
        s.run(3)
        pr = s.profile_read()
        assert {k: v["launches"] for k, v in pr.items()} == dict(walk=3, rank=0, evaporate=3, deposit=3), (r, pr)
        assert all(pr[k]["ms"] > 0 for k in ("walk", "evaporate", "deposit")), (r, pr)
    got = R.collect(s, 0, 150)
    s.close()
    R.same(got, want(150), "fifty rounds")


def test_profile_again_with_pairs_outstanding(ctx, dgrids):
    """wa_acs_profile clears the accumulators and leaves the pairs in flight alone: they are harvested by the next read, into the new figures; a
    period change and a switch-off in between lose no pair and change no result"""
    s = solver(ctx, dgrids, {}, 100)
    s.profile(True, 1)
    s.run(5)               # 5 stamped generations, not read
    s.profile(True, 2)
    s.run(10)              # generations 5 .. 14: 6, 8, 10, 12, 14 are stamped
    s.profile(False)
    s.run(5)               # nothing stamped
    s.profile(True, 10)    # accumulators cleared, 10 pairs of each class still in flight
    s.run(80)              # generations 20 .. 99: eight stamped
    pr = s.profile_read()
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=18, rank=0, evaporate=18, deposit=18), pr
    pr = s.profile_read()  # a second read harvests nothing new
    assert {k: v["launches"] for k, v in pr.items()} == dict(walk=18, rank=0, evaporate=18, deposit=18), pr
    got = R.collect(s, 0, 100)
    s.close()
    R.same(got, want(100), "again")
