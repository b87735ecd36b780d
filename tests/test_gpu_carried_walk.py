"""The carried walk (WA_CONVERGED_CARRIED_WALK).  Behind a CARRIED window -- one that committed whole and found that every ant of the
generation behind it replays the best path too -- the flush is not enqueued at all (its rows had one reader, that generation's walk), and the
walk launch of that generation, marked WA_GEN_OWED, delivers every ant as a whole replay without a draw and without the replay table.  Behind a
window that committed whole that walk launch goes out in front of the next window's verdict (WA_GEN_SPEC) and returns at its top unless the
window turns out carried.

Every comparison is bit for bit: the five trace arrays, the best cost and path, the whole field, L and node count of the last generation's ants
(R.same against the C oracle in DEV mode) and, between runs with the switch on and off, every ant's path.  A case that claims the new path
asserts from wa_acs_converged_carried_info that a walk launch took it (counted on the device) and that as many rows launches were left out as
windows were read carried; with the switch off, or on a path that does not qualify, all four counters are zero.

The searches are the ones of test_gpu_converged_run.py / test_gpu_converged_owed.py / test_gpu_converged_cycle.py, whose docstrings say which
generations are replays and which windows are carried, whole but not carried, or cut."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_converged_owed as W
import test_gpu_converged_run as R
import test_gpu_poisoned_scratch as P
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)
from test_gpu_converged_cycle import eleven  # noqa: F401
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

MINE = ("WA_CONVERGED_CARRIED_WALK", "WA_CONVERGED_SPECULATE")
ZERO = dict(walks=0, rows_skipped=0, spec_walks=0, spec_cancelled=0)
OFF = dict(WA_CONVERGED_CARRIED_WALK=0)


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in MINE}
    try:
        for k in MINE:
            os.environ.pop(k, None)
            if k in env:
                os.environ[k] = str(env[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run(ctx, dgrids, case, env, at=None, **kw):
    """W.run with the carried-walk counters and, behind the search's last generation, every ant's path and the stamps read.  at: {generations
    done: callable(s)} for reads in between.  Returns a dict: out (per slot), info, owed, cw, paths, prof"""
    gens = R.CASES[case][4]
    got = {}

    def between(s, done):
        if at and done in at:
            at[done](s)
        if done == gens:
            got["prof"] = {k: v["launches"] for k, v in s.profile_read().items()}
            got["cw"] = s.converged_carried_info()
            got["host"] = s.converged_host_info()
            if kw.get("P", 1) == 1:
                got["paths"] = [s.ant_path(a) for a in range(len(s.ants(0)[0]))]
    with switches(env):
        out, info, owed = W.run(ctx, dgrids, case, {k: v for k, v in env.items() if k not in MINE}, between=between, **kw)
    return dict(out=out, info=info, owed=owed, **got)


def same_runs(a, b, tag, info=True):
    """info: the runs place their windows alike (the same calls), so what the windows committed is equal too"""
    for q in range(len(a["out"])):
        R.same(a["out"][q], b["out"][q], (tag, q))
    assert len(a["paths"]) == len(b["paths"]) and all(np.array_equal(x, y) for x, y in zip(a["paths"], b["paths"])), (tag, "ant paths")
    assert not info or a["info"] == b["info"], (tag, a["info"], b["info"])


def on_off_oracle(ctx, dgrids, case, env, tag, **kw):
    """switch on == switch off == oracle; the new path was taken with the switch on and not at all with it off.  Returns the run with it on"""
    on = run(ctx, dgrids, case, env, **kw)
    off = run(ctx, dgrids, case, dict(env, **OFF), **kw)
    print(tag, on["info"], on["owed"], on["cw"], on["host"])
    R.same(off["out"][0], R.ref(case), (tag, "off"))
    R.same(on["out"][0], R.ref(case), (tag, "on"))
    same_runs(on, off, tag)
    assert off["cw"] == ZERO, (tag, off["cw"])
    assert on["owed"] == off["owed"], (tag, on["owed"], off["owed"])       # the counters keep their meaning
    o = on["owed"]
    assert o["merged"] == o["carried"] == o["out_of_place"] + o["in_place"], (tag, o)
    assert on["cw"]["walks"] >= 1 and on["cw"]["walks"] == o["carried"], (tag, on["cw"], o)
    assert on["cw"]["rows_skipped"] == o["carried"], (tag, on["cw"], o)
    assert on["prof"] == off["prof"], (tag, on["prof"], off["prof"])       # launches per class of the stamped generations
    return on


@pytest.mark.parametrize("period,window", [(10, None), (5, None), (10, 3)], ids=["period10", "period5", "window3"])
def test_switch_on_off_oracle(ctx, dgrids, period, window):
    """windows of nine and of four generations between stamped ones (both parities of the paying sweep), and chains of windows of three of which
    only the last has a full generation behind it"""
    env = {} if window is None else dict(WA_CONVERGED_WINDOW=window)
    on = on_off_oracle(ctx, dgrids, "firm", env, ("firm", period, window), profile=period)
    if window is None:
        assert on["owed"]["out_of_place"] >= 1 and on["owed"]["in_place"] >= 1, on["owed"]
        assert on["cw"]["spec_walks"] >= 1, on["cw"]                      # behind a whole window the walk goes out ahead of the verdict
    assert sum(on["prof"].values()) > 0, on["prof"]


def test_the_two_float_tail(ctx, dgrids, eleven):
    """11^3: the paying sweep's tail of two floats behind windows that left no rows"""
    on_off_oracle(ctx, dgrids, eleven, {}, "eleven", profile=10)


def test_ants_of_a_carried_generation(ctx, dgrids):
    """firm, stamped every 10th generation: a call of 61 generations ends on generation 60, the one behind the carried window 51-59.  Its ants are
    what the carried walk wrote: every one the best path, with its cost"""
    seen = {}

    def read(s):
        s.sync()
        cost, path, _ = s.result(0)
        L, lens = s.ants(0)
        seen.update(cost=cost, path=path, L=L, lens=lens, paths=[s.ant_path(a) for a in range(len(L))], cw=s.converged_carried_info(),
                    owed=s.converged_owed_info())
    on = run(ctx, dgrids, "firm", {}, at={61: read}, pieces=[61], profile=10)
    R.same(on["out"][0], R.ref("firm"), "ants, the whole search")
    assert seen["cw"]["walks"] >= 1 and seen["cw"]["walks"] == seen["owed"]["merged"], seen["cw"]   # generation 60 was a carried walk
    assert len(seen["L"]) == R.CASES["firm"][2]
    assert np.array_equal(R.bits(seen["L"]), np.full(len(seen["L"]), R.bits(seen["cost"]), np.uint32)), seen["L"]
    assert (seen["lens"] == len(seen["path"])).all(), seen["lens"]
    assert all(np.array_equal(p, seen["path"]) for p in seen["paths"])
    n, occ, colony, rho, _, seed = R.CASES["firm"]
    g, (sid, eid) = R.ogrid(n, occ)
    a = O.Acs(g)
    a.solve(sid, eid, 61, float(colony / 0.35), fixed_colony=colony, mode=O.DEV, seed=seed, stream=0, rho=rho)
    lens, L = a.last_ants()
    assert np.array_equal(R.bits(L), R.bits(seen["L"])) and np.array_equal(lens, seen["lens"])
    assert np.array_equal(a.best_path()[0], seen["path"])


def test_whole_but_not_carried(ctx, dgrids):
    """rho 0.9, calls of 70, 4 and 26: window 64-68 is carried into generation 69; window 70-72 commits whole and an ant leaves the path in
    generation 73 -- the walk enqueued ahead returns at its top and today's flush follows the verdict"""
    on = on_off_oracle(ctx, dgrids, "partial", {}, "partial 70 4 26", pieces=[70, 4, 26], stragglers=0)
    assert on["owed"]["fallback"] >= 1 and on["cw"]["spec_cancelled"] >= 1, (on["owed"], on["cw"])


def test_a_cut_window_directly_behind_a_whole_one(ctx, dgrids):
    """rho 0.9, stamped every 4th generation: 73-75 commits nothing behind the carried 69-71, 85-87 one generation, 93-95 two"""
    on = on_off_oracle(ctx, dgrids, "partial", {}, "partial period 4", profile=4, stragglers=0)
    assert on["info"][0]["cut"] > 0 and on["owed"]["carried"] >= 5 and on["cw"]["spec_cancelled"] >= 1, (on["info"], on["owed"], on["cw"])
    assert on["host"][2] >= 1, on["host"]


def test_uneven_calls_with_and_without_reads(ctx, dgrids):
    pieces = [7, 1, 13, 2, 27]
    whole = run(ctx, dgrids, "firm", {}, profile=10)
    plain = run(ctx, dgrids, "firm", {}, profile=10, pieces=pieces)
    fields = {}

    def read(done):
        def f(s):
            s.sync()
            fields[done] = R.bits(s.pheromone(0)).copy()
            s.ants(0)
        return f
    reads = run(ctx, dgrids, "firm", {}, profile=10, pieces=pieces, at={d: read(d) for d in np.cumsum(pieces).tolist()})
    for r, tag in ((whole, "one call"), (plain, "pieces"), (reads, "pieces, read")):
        R.same(r["out"][0], R.ref("firm"), tag)
        assert r["cw"]["walks"] >= 1 and r["cw"]["rows_skipped"] == r["owed"]["carried"] == r["cw"]["walks"], (tag, r["cw"], r["owed"])
    same_runs(whole, plain, "one call == pieces", info=False)             # (a window never covers the last generation of a call)
    same_runs(plain, reads, "pieces == pieces with reads")
    assert np.array_equal(fields[50], W.field_after("firm", 50))          # 7 + 1 + 13 + 2 + 27: behind generation 49


@pytest.mark.parametrize("env,path", [(dict(WA_CONVERGED_SPECULATE=0), True), (dict(WA_CONVERGED_OWED=0), False)], ids=["no speculation", "nothing owed"])
def test_neighbouring_switches(ctx, dgrids, env, path):
    r = run(ctx, dgrids, "firm", env, profile=10)
    R.same(r["out"][0], R.ref("firm"), sorted(env.items()))
    if path:   # the walk is never enqueued ahead; the rows launch of a window read as carried is still left out
        assert r["cw"]["spec_walks"] == r["cw"]["spec_cancelled"] == 0, r["cw"]
        assert r["cw"]["walks"] >= 1 and r["cw"]["walks"] == r["cw"]["rows_skipped"] == r["owed"]["carried"], (r["cw"], r["owed"])
    else:
        assert r["cw"] == ZERO, r["cw"]


@pytest.mark.parametrize("kw", [dict(P=2, groups=1), dict(P=2, groups=2), dict(lazy=True), dict(nb=26)], ids=["batch", "groups", "lazy", "nb26"])
def test_paths_that_do_not_qualify(ctx, dgrids, kw):
    r = run(ctx, dgrids, "firm", {}, profile=10, **kw)
    for q in range(len(r["out"])):
        R.same(r["out"][q], R.ref("firm", q, kw.get("nb", 6)), (sorted(kw.items()), q))
    assert r["cw"] == ZERO, r["cw"]


def test_ref_mode_does_not_qualify(ctx, dgrids):
    n, occ, colony, rho, gens, seed = R.CASES["firm"]
    g, (sid, eid) = R.ogrid(n, occ)
    s = api.AcsSolver(ctx, dgrids(n, occ), n_slots=1, max_colony=colony)
    s.srand(seed)
    s.solve(api.default_params(max_iteration=gens, predict=float(colony / 0.35), fixed_colony=colony, rng_mode=api.RNG_REF, rho=rho), [sid], [eid])
    s.sync()
    cw, t = s.converged_carried_info(), s.trace(0)
    field = R.bits(s.pheromone(0))
    s.close()
    a = O.Acs(g)
    tr = a.solve(sid, eid, gens, float(colony / 0.35), fixed_colony=colony, mode=O.REF, rng=O.srand(seed), rho=rho)
    assert np.array_equal(R.bits(t["bestL"][:gens]), R.bits(tr["bestL"])) and np.array_equal(t["steps"][:gens], tr["steps"])
    assert np.array_equal(field, R.bits(a.pheromone()))
    assert cw == ZERO, cw


def test_null_safe(ctx):
    out = (api.C.c_uint64 * 4)()
    assert ctx.lib.wa_acs_converged_carried_info(None, out) != 0


@pytest.mark.parametrize("byte", P.BYTES, ids=lambda b: "byte%02x" % b)
def test_poisoned_allocations_red_zones_and_leaks(byte):
    """every device block filled with 0xff / 0x55 before it is handed out, red zones round it: the rows that are no longer written must not be
    read, nothing is written outside a block, and nothing is left behind close()"""
    c = P.make_ctx(WA_DEV_POISON=1, WA_DEV_POISON_BYTE=byte, WA_DEV_GUARD=1, WA_DEV_GUARD_BYTE=P.GUARD_BYTE[byte])
    made = {}

    def grids(n, occ):
        if (n, occ) not in made:
            g, _ = R.ogrid(n, occ)
            made[(n, occ)] = api.Grid.from_occupancy(c, g.free, g.cx, g.cy, g.cz, g.precision, g.wall)
        return made[(n, occ)]
    try:
        for period in (10, 5):
            r = run(c, grids, "firm", {}, profile=period)
            R.same(r["out"][0], R.ref("firm"), ("poisoned", byte, period))
            assert r["cw"]["walks"] >= 1 and r["cw"]["rows_skipped"] == r["owed"]["carried"] == r["cw"]["walks"], (r["cw"], r["owed"])
        for dg in made.values():
            dg.close()
        c.trim()
        s = c.guard_stats()
        assert s["live_blocks"] == 0 and s["live_bytes"] == 0 and s["front_damaged"] + s["back_damaged"] == 0 and s["checked"] > 0, s
    finally:
        c.close()
