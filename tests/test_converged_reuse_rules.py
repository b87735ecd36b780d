"""What test_gpu_converged_reuse.py claims of the converged cycle's counters, held against the C oracle alone (no GPU).

For every scenario of converged_reuse_ref.py and every search in it, F.expect() names, from the oracle's trace rows (a necessary condition), the last
window that must commit a generation and the last one that must be carried.  Here the oracle sequence is played again up to each generation those
claims use, and every ant's path of that generation compared with the best path (F.is_replay, the sufficient condition): the first generation of the
committing window, and every generation of the carried window and the one behind it.  A claim that does not hold fails here, so that the counter
assertions on the GPU are never vacuous and never wrong; the scenario (a seed, a length) is changed then, not the assertion."""
import numpy as np
import pytest

import converged_reuse_ref as F
import oracle_lib as O

SEARCHES = [(name, slot, s.index) for name, sc in F.SCENARIOS.items() for slot in range(sc.n_slots) for s in F.play(name, slot) if s.want is not None]


@pytest.mark.parametrize("name,slot,index", SEARCHES, ids=lambda v: str(v))
def test_claimed_generations_are_replays(name, slot, index):
    e = F.expect(name, slot, index)
    rows = set(F.replays(name, slot, index))
    if e["commit"] is not None:
        assert e["commit"] in rows and F.is_replay(name, slot, index, e["commit"]), (name, slot, index, e["commit"])
    if e["carried"] is not None:
        g0, w = e["carried"]
        assert (g0, w, True) in e["windows"]
        for g in range(g0, g0 + w + 1):
            assert g in rows and F.is_replay(name, slot, index, g), (name, slot, index, g)


def test_a_claim_outside_the_evidence_fails():
    """generation 34 of firm: its trace row already says that an ant left the path; generations 21 and 22 pass the trace row and fail the paths"""
    assert 34 not in F.replays("par_plain", 0, 0) and not F.is_replay("par_plain", 0, 0, 34)
    for g in (21, 22):
        assert g in F.replays("par_plain", 0, 0) and not F.is_replay("par_plain", 0, 0, g)
    assert F.is_replay("par_plain", 0, 0, 25) and F.is_replay("par_plain", 0, 0, 99)


def test_the_lists_of_the_first_test_file():
    """firm on a fresh solver: the replay generations test_gpu_converged_run.py's docstring lists (found the same way)"""
    want = {25, 27} | set(range(29, 34)) | set(range(35, 100))
    assert F.all_replays("par_plain", 0, 0) == want


def test_every_scenario_claims_what_it_is_there_for():
    """the searches a scenario is there for claim windows that commit -- and, lone and read by the host, carried ones"""
    def claims(name, index, slot=0):
        e = F.expect(name, slot, index)
        return e["commit"] is not None, e["carried"] is not None
    for W in (5, 40, 61, 100):
        assert claims("warmup%d" % W, 1) == (True, True)
    for k in (26, 34, 60, 61, 73):
        for tail in ("", "_result"):
            assert claims("abandoned%d%s" % (k, tail), 1) == (True, True)
    for name in ("continuing", "continuing_no_stragglers"):     # (the hand-over of stragglers on and off)
        assert claims(name, 0) == claims(name, 1) == (True, True) and claims(name, 2)[0], name
    assert claims("continuing_partial", 1) == (True, True)
    assert claims("modes", 1) == (False, False) and claims("modes", 0) == claims("modes", 2) == claims("modes", 3) == (True, True)
    for n in (99, 100):
        assert all(claims("lone%d" % n, 1, q) == (True, False) for q in range(3)) and claims("lone%d" % n, 2)[0]
    assert claims("lone100", 0) == (True, True) and claims("lone99", 0) == (True, False)
    assert all(claims("colony_and_rho", i)[0] for i in range(4)) and claims("colony_and_rho", 1) == (True, True)
    assert all(claims("profiling", i) == (True, True) for i in range(3))
    for name in F.PARAMETERS:
        if name != "alpha0":
            assert claims("par_" + name, 0) == (True, True), name
    assert claims("par_alpha0", 0) == (False, False)


def test_windows_follow_the_documented_placement():
    """DESIGN 4p, "Which generations": one call of 100 generations, stamped every 10th and not; calls of 1 and 79; a call of 61"""
    assert F.windows((100,)) == [(0, 32, False), (32, 32, False), (64, 32, False), (96, 3, True)]
    assert F.windows((100,), 10) == [(g, 9, True) for g in range(1, 90, 10)] + [(91, 8, True)]
    assert F.windows((1, 79)) == [(1, 32, False), (33, 32, False), (65, 14, True)]
    assert F.windows((1, 66, 13)) == [(1, 32, False), (33, 32, False), (65, 1, False), (67, 12, True)]
    assert F.windows((67, 13)) == [(0, 32, False), (32, 32, False), (64, 2, False), (67, 12, True)]
    assert F.windows((61,), 10)[-1] == (51, 9, True) and F.windows((2,)) == [(0, 1, False)] and F.windows((1,)) == []


def test_continued_searches_replay_from_generation_1():
    """a search begun on a trained field: its best path dates from its generation 0 and every later generation is a replay"""
    assert F.all_replays("continuing_no_stragglers", 0, 1) == frozenset(range(1, 80))
    assert F.exact("continuing_no_stragglers", 0, 1) == dict(enqueued=4, whole=4, cut=0, generations=77)
    p = F.play("continuing_no_stragglers", 0)
    assert len(p[2].want["path"]) != len(p[0].want["path"])     # the reversed ends settle on another path
    assert p[1].first is None and p[0].first == ("init", 1.0)


def test_an_init_step_equals_a_new_oracle():
    """the player's init step (a new oracle object) and reset step against oracle runs written out by hand"""
    g, (sid, eid) = F.grid("c2")
    a = O.Acs(g)
    a.solve(sid, eid, 40, 50 / 0.35, fixed_colony=50, mode=O.DEV, seed=1007, rho=0.8)
    b = O.Acs(g)
    b.solve(sid, eid, 100, 50 / 0.35, fixed_colony=50, mode=O.DEV, seed=7, rho=0.8)
    assert np.array_equal(F.play("warmup40", 0)[1].want["field"], F.R.bits(b.pheromone()))
    a.reset(1.0)                       # a reset field on a used oracle == a reset field on a new one (every edge p0); != an init field
    a.solve(sid, eid, 100, 50 / 0.35, fixed_colony=50, mode=O.DEV, seed=7, stream=1, rho=0.8)
    got = F.play("abandoned26", 0)[1].want
    assert np.array_equal(got["field"], F.R.bits(a.pheromone())) and not np.array_equal(got["field"], F.R.ref("firm", 1)["field"])
    assert np.array_equal(got["bestL"], F.R.ref("firm", 1)["bestL"])          # (the edges out of bounds are never walked)
    behind_reset, behind_init = F.play("modes", 0)[2].want, F.play("modes", 0)[3].want
    assert all(np.array_equal(behind_reset[k], v) for k, v in got.items())
    assert all(np.array_equal(behind_init[k], v) for k, v in F.R.ref("firm", 1).items())
