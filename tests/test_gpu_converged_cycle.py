"""The cycle of a converged search -- window kernel, flush, stamped full generation -- at shapes of its device ends that no test visited.

1. The sweep behind a carried window (wa_sweep_body_nt with several multiplications a value, csrc/acs_update.hpp) at every mix of trips a thread its
loops can meet, the two-float tail included.
2. A window that meets a colony out of range (k_converged_run's control chain, csrc/acs_converged.hpp).
(Two changes to these kernels were measured beside them and not kept, profiles/converged_cycle/README.md; the cases stay.)

Every case is held bit for bit over the five trace arrays, the best cost and path, the ants of the last generation and the WHOLE pheromone field
against the C oracle in DEV mode, through the harness of test_gpu_converged_run.py / test_gpu_converged_owed.py, and asserts from the info counters
that the path it is there for was taken.

The 12^3 search `firm` has 6 x 1 728 = 10 368 values, 2 592 float4.  With WA_EVAP_BLOCKS = 1, 3, 4 and the default (4 096) a thread of the 256-thread
sweep blocks has 10.1, 3.4, 2.5 and at most one trip: two rounds of four and a ragged third, the ragged mix a 128^3 field has at 4 096 blocks (three trips
every thread: the loop of four never runs), and the single trip.  Stamped every 10th generation the merged sweeps multiply 10 times (in place) and, in
front of the last generation, 9 times (out of place); every 5th: 5 (out of place) and 4 (in place) -- see test_gpu_converged_owed.py.

`eleven` is `firm` on an 11^3 grid: 6 x 1 331 = 7 986 values, no multiple of four, so the two-float tail runs with several multiplications.  The oracle
alone (every ant of a generation compared with the best path, as described in test_gpu_converged_run.py) says its replay generations include 36-99
without a gap: stamped every 10th generation the windows 41-49, ..., 81-89 and 91-98 are carried into generations 50, ..., 90 and 99.

A colony cannot leave its range INSIDE a window: a generation's colony is a function of the best cost, which no committed generation changes, so the
chain either stops at its first step or never.  The case that exists is `nearby`: start and end two steps apart, the colony sized from the best cost (no
fixed colony): 21 ants, then 1, 1 (generation 2 finds the two-step path) and 0 from generation 3 on, says the oracle.  With windows of three, every window
from generation 3 on meets a colony of 0 at its first generation and commits nothing."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_converged_owed as W
import test_gpu_converged_run as R
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

KEYS = ("WA_EVAP_BLOCKS", "WA_CONVERGED_WINDOW")
CASES = {"eleven": (11, 0.02, 50, 0.8, 100, 7)}


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
            if env.get(k) is not None:
                os.environ[k] = str(env[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eleven():
    """`eleven` beside the cases of test_gpu_converged_run.py for the time of this module (R.gpu and R.ref look their case up by name)"""
    R.CASES.update(CASES)
    yield "eleven"
    for k in CASES:
        R.CASES.pop(k, None)


def merged_sweeps(ctx, dgrids, case, blocks, period):
    """the search with `blocks` sweep blocks == oracle; the owed counters of the run"""
    with switches(dict(WA_EVAP_BLOCKS=blocks)):
        on, info, owed = W.run(ctx, dgrids, case, {}, profile=period)
    R.same(on[0], R.ref(case), (case, blocks, period))
    assert owed["merged"] == owed["carried"] == owed["out_of_place"] + owed["in_place"], owed
    return owed


@pytest.mark.parametrize("period", [10, 5])
@pytest.mark.parametrize("blocks", [1, 3, 4, None])
def test_merged_sweeps_by_trips_a_thread(ctx, dgrids, blocks, period):
    """10 / 9 and 5 / 4 multiplications a value at about 10, 3.4, 2.5 and at most one trip a thread"""
    owed = merged_sweeps(ctx, dgrids, "firm", blocks, period)
    if period == 10:
        assert owed["in_place"] >= 5 and owed["out_of_place"] >= 1, owed      # 50, 60, 70, 80, 90; 99
    else:
        assert owed["out_of_place"] >= 5 and owed["in_place"] >= 1, owed      # 45, 50, 55, ...; 99 behind window 96-98


@pytest.mark.parametrize("blocks", [1, 3, None])
def test_the_two_float_tail_with_several_multiplications(ctx, dgrids, eleven, blocks):
    """11^3: 7 986 values = 1 996 float4 and a tail of two, which thread 0 and 1 of sweep block 0 multiply 10 and 9 times"""
    owed = merged_sweeps(ctx, dgrids, eleven, blocks, 10)
    assert owed["in_place"] >= 5 and owed["out_of_place"] >= 1, owed          # 50, 60, 70, 80, 90; 99


def nearby(ctx, dgrids):
    n, occ, gens = 12, 0.02, 30
    g, (sid, _) = R.ogrid(n, occ)
    eid = g.resolve(g.node_pt(2, 2, 4))
    with switches(dict(WA_CONVERGED_WINDOW=3)):
        s = api.AcsSolver(ctx, dgrids(n, occ), n_slots=1, max_colony=32)
    s.begin(api.default_params(max_iteration=gens, predict=60.0, fixed_colony=0, rng_mode=api.RNG_DEV, seed=7, rho=0.8), [sid], [eid], streams=[0])
    s.run(gens)
    s.sync()
    got, info = R.collect(s, 0, gens), s.converged_info(0)
    s.close()
    return got, info


def test_a_colony_out_of_range_ends_the_window_at_once(ctx, dgrids):
    """`nearby`: from generation 3 on the colony is 0 and every window (of three generations) stops in front of its first generation"""
    n, occ, gens = 12, 0.02, 30
    g, (sid, _) = R.ogrid(n, occ)
    eid = g.resolve(g.node_pt(2, 2, 4))
    a = O.Acs(g)
    tr = a.solve(sid, eid, gens, 60.0, fixed_colony=0, mode=O.DEV, seed=7, stream=0, rho=0.8)
    assert tr["colony"][:4].tolist() == [21, 1, 1, 0] and not tr["colony"][3:].any(), tr["colony"]
    lens, L = a.last_ants()
    want = dict(steps=tr["steps"], finite=tr["finite"], colony=tr["colony"], bestL=R.bits(tr["bestL"]), iterbestL=R.bits(tr["iterbestL"]),
                cost=R.bits(a.best_L), path=a.best_path()[0], field=R.bits(a.pheromone()), antL=R.bits(L), antLen=lens)
    got, info = nearby(ctx, dgrids)
    R.same(got, want, "nearby")
    # windows of three are placed at generations 0, 3, ..., 27 whatever they commit: the first finds no best path yet, the nine others a colony of 0
    assert info == dict(enqueued=10, whole=0, cut=0, generations=0), info
