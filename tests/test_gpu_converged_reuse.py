"""The converged cycle in a solver that is used for more than one search: bench.py's warm-up, an abandoned search, a search that
continues on a trained field, DEV / REF / DEV, a lone search in a wide solver, colonies and rho that change, profiling toggled, parameters off their
defaults -- the scenarios of converged_reuse_ref.py, whose docstring describes the steps.

Every search that is read is compared bit for bit (R.same: the five trace arrays, the best cost and path, the WHOLE field, L and node count of the
last ants; for a lone search every ant's path too) with
  (a) the C oracle playing the same sequence of searches (F.play),
  (b) the same sequence on a solver created with WA_CONVERGED_RUN=0,
  (c) where the search starts from an init or reset field, the same search on a fresh solver.
The counters of converged_info, converged_host_info, converged_owed_info and converged_carried_info run since the solver was created, so they are
read behind every wa_acs_begin (which drains the stream and moves none of them) and behind the search, and the DIFFERENCES are asserted:
  * windows enqueued == the windows the documented placement gives (F.windows), per slot; idle slots move nothing;
  * where the oracle says the last window begins with a replay: generations > 0; where it says a judged window and the generation behind it are
    replays: a carried walk and an owed merge (F.expect; test_converged_reuse_rules.py confirms each such claim with the oracle alone);
  * for the searches in F.EXACT, whole / cut / generations as the oracle's replay generations give them (F.exact);
  * a search from an init / reset field moves every counter exactly as on the fresh solver, and stamps as many launches per class;
  * a REF search moves nothing; a batch moves none of the host's counters; with the switch off everything stays 0."""
import contextlib
import os

import numpy as np
import pytest

import converged_reuse_ref as F
import oracle_lib as O
import test_gpu_carried_walk as CW
import test_gpu_converged_owed as W
import test_gpu_converged_run as R
import test_gpu_poisoned_scratch as P
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

ZERO_INFO = dict(enqueued=0, whole=0, cut=0, generations=0)


@contextlib.contextmanager
def environment(env):
    """the switches a solver reads when it is created: R.KEYS as R.gpu sets them, the others through their modules' own handling"""
    old = {k: os.environ.get(k) for k in R.KEYS}
    try:
        for k in R.KEYS:
            os.environ.pop(k, None)
            if k in env:
                os.environ[k] = str(env[k])
        with W.switches(env), CW.switches(env):
            yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def grids(ctx, dgrids):
    """device grid of a scenario: the 12^3 ones from R's dgrids, the 13 x 11 x 9 box made here"""
    yield grid_maker(ctx, dgrids)


def grid_maker(c, cubes=None):
    made = {}

    def get(key):
        if cubes is not None and key in ("c2", "c5"):
            return cubes(12, 0.02 if key == "c2" else 0.05)
        if key not in made:
            g, _ = F.grid(key)
            made[key] = api.Grid.from_occupancy(c, g.free, g.cx, g.cy, g.cz, g.precision, g.wall)   # (closed with its context)
        return made[key]
    get.made = made
    return get


def counters(s, n_slots):
    """every counter of the mechanism (converged_info and converged_carried_info wait for the stream; none of them drains stragglers or reads results)"""
    return dict(info=[s.converged_info(q) for q in range(n_slots)], host=s.converged_host_info(), owed=s.converged_owed_info(), cw=s.converged_carried_info())


def minus(a, b):
    return dict(info=[{k: x[k] - y[k] for k in x} for x, y in zip(a["info"], b["info"])], host=[x - y for x, y in zip(a["host"], b["host"])],
                owed={k: a["owed"][k] - b["owed"][k] for k in a["owed"]}, cw={k: a["cw"][k] - b["cw"][k] for k in a["cw"]})


def drive(c, grids, sc, env):
    """the steps of a scenario on one solver.  Returns one dict per begin step: out (collect per slot of the batch, None where the search is not
    read), paths (every ant's path, a lone search), delta (the counters' differences across the search), prof (launches per class, stamped),
    idle ({slot: its field}, slots outside the batch), restarted (wa_acs_profile was called between the search before and this one) -- and the
    counters behind the last step"""
    g, (sid, eid) = F.grid(sc.grid)
    with environment(env):
        s = api.AcsSolver(c, grids(sc.grid), n_slots=sc.n_slots, max_colony=sc.max_colony)
    s.set_pipeline(1)
    got, cur, period, restarted = [], None, 0, False
    try:
        for st in sc.steps:
            op = st[0]
            if op == "init":
                s.init_pheromone(st[1], st[2] if len(st) > 2 else -1)
            elif op == "reset":
                s.reset_pheromone(st[1], st[2] if len(st) > 2 else -1)
            elif op == "begin":
                b = st[1]
                P_ = len(b["streams"])
                a, z = (eid, sid) if b["rev"] else (sid, eid)
                if b["mode"] == O.REF:
                    s.srand(b["seed"])
                p = api.default_params(max_iteration=b["max_iteration"], predict=float(b["colony"] / 0.35), fixed_colony=b["colony"], seed=b["seed"],
                                       rng_mode=api.RNG_DEV if b["mode"] == O.DEV else api.RNG_REF, rho=b["rho"], alpha=b["alpha"], beta=b["beta"],
                                       pheromone_0=b["pheromone_0"])
                s.begin(p, [a] * P_, [z] * P_, streams=list(b["streams"]))
                cur = dict(P=P_, done=0, before=counters(s, sc.n_slots), out=None, period=period, restarted=restarted)
                got.append(cur)
            elif op == "run":
                s.run(st[1])
                cur["done"] += st[1]
                restarted = False
            elif op == "read":
                s.sync()
                cur["out"] = [R.collect(s, q, cur["done"]) for q in range(cur["P"])]
                if cur["P"] == 1:
                    cur["paths"] = [s.ant_path(k) for k in range(len(s.ants(0)[0]))]
                if cur["period"]:
                    cur["prof"] = {k: v["launches"] for k, v in s.profile_read().items()}
                cur["idle"] = {q: R.bits(s.pheromone(q)) for q in range(cur["P"], sc.n_slots)}
                cur["delta"] = minus(counters(s, sc.n_slots), cur["before"])
            elif op == "result":
                s.result(0)
            elif op == "profile":
                period = st[1]
                s.profile(period > 0, max(period, 1))      # (also sets the launches per class back to 0)
                restarted = True
                if cur is not None and not cur["done"]:
                    cur["period"], cur["restarted"] = period, True
            elif op == "evaporate":
                s.evaporate(0, st[1], st[2])
            elif op == "stragglers":
                s.set_stragglers(st[1])
            else:
                raise AssertionError(op)
        s.sync()
        return got, counters(s, sc.n_slots)
    finally:
        s.close()


def fresh(name, index):
    """the steps of search `index` alone, as a scenario for a new solver of the search's own size -- or None where a slot of it continues on a
    trained field"""
    sc = F.SCENARIOS[name]
    s0 = F.play(name, 0)[index]
    P_ = len(s0.begin["streams"])
    firsts = [F.play(name, q)[index].first for q in range(P_)]
    if any(f is None for f in firsts):
        return None
    steps = [(op, p0, q) for q, (op, p0) in enumerate(firsts)]
    if s0.stragglers is not None:
        steps.append(("stragglers", s0.stragglers))
    if s0.period:
        steps.append(("profile", s0.period))
    steps += [("begin", s0.begin)] + [("run", k) for k in s0.pieces] + [("read",)]
    return F.Scenario(sc.grid, P_, s0.begin["colony"], steps)


def check(c, grids, name, off=True, alone=True):
    """(a), (b), (c) and the counters for every search of the scenario; returns the searches of the run with the mechanism on"""
    sc = F.SCENARIOS[name]
    on, _ = drive(c, grids, sc, {})
    runs = [("on", on)]
    if off:
        got_off, total_off = drive(c, grids, sc, dict(WA_CONVERGED_RUN=0))
        runs.append(("off", got_off))
        assert all(i == ZERO_INFO for i in total_off["info"]) and not any(total_off["host"]), (name, total_off)
        assert total_off["owed"] == W.NONE and total_off["cw"] == CW.ZERO, (name, total_off)
    plays = [F.play(name, q) for q in range(sc.n_slots)]
    for i, g in enumerate(on):
        s0 = plays[0][i]
        assert (g["out"] is not None) == s0.read and g["done"] == s0.gens, (name, i)
        if not s0.read:
            continue
        P_ = g["P"]
        for tag, got in runs:                                               # (a), (b)
            for q in range(P_):
                R.same(got[i]["out"][q], plays[q][i].want, (name, i, tag, q))
            if P_ == 1:
                assert len(got[i]["paths"]) == len(s0.paths) and all(np.array_equal(x, y) for x, y in zip(got[i]["paths"], s0.paths)), (name, i, tag, "ant paths")
            for q, f in got[i]["idle"].items():
                assert np.array_equal(f, plays[q][i].field), (name, i, tag, "idle slot", q)
        d = g["delta"]
        print(name, i, d)
        dev = s0.begin["mode"] == O.DEV
        for q in range(sc.n_slots):
            e = F.expect(name, q, i) if q < P_ else None
            if not dev or e is None:
                assert d["info"][q] == ZERO_INFO, (name, i, q, d["info"][q])   # a REF search, a slot outside the batch
                continue
            assert d["info"][q]["enqueued"] == len(e["windows"]) > 0, (name, i, q, d["info"][q], e["windows"])
            if e["commit"] is not None:
                assert d["info"][q]["generations"] > 0, (name, i, q, d["info"][q], e)
            if e["carried"] is not None:
                assert d["cw"]["walks"] >= 1 and d["owed"]["merged"] >= 1 and d["owed"]["carried"] >= 1, (name, i, d, e)
            if (name, i) in F.EXACT:
                assert d["info"][q] == F.exact(name, q, i), (name, i, q, d["info"][q], F.exact(name, q, i))
        if not dev or P_ > 1:                                               # nothing is read back, judged or owed
            assert not any(d["host"]) and d["owed"] == W.NONE and d["cw"] == CW.ZERO, (name, i, d)
        else:
            o = d["owed"]
            assert o["merged"] == o["carried"] == o["out_of_place"] + o["in_place"] == d["cw"]["walks"] == d["cw"]["rows_skipped"], (name, i, d)
            assert d["host"][0] > 0 and d["host"][3] == 0, (name, i, d["host"])        # verdicts were read, no wait given up
        alone_sc = fresh(name, i) if alone else None
        if alone_sc is not None:                                            # (c)
            (f,), total = drive(c, grids, alone_sc, {})
            for q in range(P_):
                R.same(g["out"][q], f["out"][q], (name, i, "fresh", q))
            if P_ == 1:
                assert all(np.array_equal(x, y) for x, y in zip(g["paths"], f["paths"])), (name, i, "fresh", "ant paths")
            dd = dict(d, info=d["info"][:P_])
            assert dd == f["delta"] == total, (name, i, "counters on a fresh solver", dd, f["delta"], total)
            if g["restarted"]:   # (otherwise the stamps of the searches before are in the sums too: they run since wa_acs_profile was called)
                assert g.get("prof") == f.get("prof"), (name, i, g.get("prof"), f.get("prof"))
    return on


@pytest.mark.parametrize("W_", [5, 40, 61, 100])
def test_warm_up_then_the_timed_search(ctx, grids, W_):
    """bench.py: a throw-away search of W generations (no window yet; in the middle of chained windows; ending on the generation behind a carried
    window; a whole search), sync, init, the timed search -- which equals R.ref("firm") and the fresh solver, counters included.  W < 100: begin
    re-allocates the trace buffers for the second search"""
    on = check(ctx, grids, "warmup%d" % W_)
    R.same(on[1]["out"][0], R.ref("firm"), ("warm-up", W_))
    assert sum(on[1]["prof"].values()) > 0, on[1]["prof"]


@pytest.mark.parametrize("result", [False, True], ids=["unread", "result"])
@pytest.mark.parametrize("k", [26, 34, 60, 61, 73])
def test_an_abandoned_search(ctx, grids, k, result):
    """begin(max_iteration = 100) and run(k) only -- then, with no sync and no read (or with a result() read), reset and the next search on another
    stream.  firm stamped every 10th: k = 26 / 34 end inside the first committing windows, 60 / 61 on and behind the carried window 51-59; partial in
    calls of 70 and 4 ends on generation 73, behind a window that was whole but not carried"""
    check(ctx, grids, "abandoned%d%s" % (k, "_result" if result else ""))


@pytest.mark.parametrize("name", ["continuing", "continuing_no_stragglers", "continuing_partial"])
def test_continuing_on_the_trained_field(ctx, grids, name):
    """no reset between the searches: the next one replays from its generation 1, and a window stands in front of that generation (a best path that
    dates from the search's generation 0); then the reversed ends, which settle on another path; the hand-over of stragglers at its default and off"""
    on = check(ctx, grids, name)
    if name == "continuing_no_stragglers":
        assert on[1]["delta"]["info"][0] == dict(enqueued=4, whole=4, cut=0, generations=77), on[1]["delta"]


def test_modes_in_turn(ctx, grids):
    """DEV, reset, REF (srand, against the oracle in REF mode: no counter moves), reset, DEV on stream 1; then init and that search again, which
    equals R.ref("firm", 1), the whole field included (behind a reset the edges out of bounds hold p0, so only the oracle's play is the reference)"""
    on = check(ctx, grids, "modes")
    R.same(on[3]["out"][0], R.ref("firm", 1), "modes, behind the init")
    skip = ("field",)
    R.same({k: v for k, v in on[2]["out"][0].items() if k not in skip}, {k: v for k, v in R.ref("firm", 1).items() if k not in skip}, "modes, behind the reset")


@pytest.mark.parametrize("n", [99, 100])
def test_a_lone_search_in_a_wide_solver(ctx, grids, n):
    """three slots: firm alone in slot 0 (verdicts read back) for 99 and for 100 generations -- both parities of flips and of committed generations --
    while slots 1 and 2 sit out and keep their init field; then a batch of three with slot 0 reset, every slot against its own oracle run and its
    own counters; then slot 0 alone again, on its trained field"""
    on = check(ctx, grids, "lone%d" % n)
    g, _ = F.grid("c2")
    assert np.array_equal(on[0]["idle"][1], R.bits(O.Acs(g).pheromone())) and np.array_equal(on[2]["idle"][2], R.ref("firm", 2)["field"])
    for q in (1, 2):
        R.same(on[1]["out"][q], R.ref("firm", q), ("batch", q))
    assert len({i["generations"] for i in on[1]["delta"]["info"]}) > 1, on[1]["delta"]      # the streams settle at different generations


def test_colony_and_rho_change(ctx, grids):
    """one solver of 64 ants: wide (64), small (20, in calls of 67 and 13 generations), firm (50), firm at rho 0.9 on the trained field -- blocks
    and lanes are dealt anew under an unchanged scratch block"""
    check(ctx, grids, "colony_and_rho")


def test_profiling_toggled(ctx, grids):
    """stamped every 10th, not at all, every 5th; stand-alone evaporations in front of the resets flip the buffers once and three times.  The third
    search stamps as many launches per class as a fresh solver"""
    on = check(ctx, grids, "profiling")
    assert "prof" not in on[1] and sum(on[2]["prof"].values()) > sum(on[0]["prof"].values()) > 0, (on[0].get("prof"), on[2].get("prof"))


@pytest.mark.parametrize("name", sorted(n for n in F.SCENARIOS if n.startswith("par_")))
def test_parameters(ctx, grids, name):
    """alpha 2 and 3 (no stragglers, no 16-bit tabu entries; also stamped every 10th, so that carried walks and owed sweeps occur there), beta 0.3 and
    0.9, rho 0.5, pheromone_0 0.25, the 13 x 11 x 9 grid at precision 0.0173; alpha 0 never converges: windows are enqueued and commit nothing.
    The alpha 2 and alpha 3 cases are the regression test of a fault these tests found: k_walk_dev's instantiations for alpha != 1 stepped over the
    carried path, so the walk behind a carried window read rows nobody had written and the launch sent ahead of the verdict did nothing while the
    host counted it as run -- walks stayed 0 beside rows_skipped 1 (one call) and 9 (stamped every 10th), which check() holds equal"""
    on = check(ctx, grids, name, alone=False)
    if "alpha0" in name:
        i = on[0]["delta"]["info"][0]
        assert i["enqueued"] > 0 and i["whole"] == i["cut"] == i["generations"] == 0, i


@pytest.mark.parametrize("byte", P.BYTES, ids=lambda b: "byte%02x" % b)
def test_poisoned_allocations_red_zones_and_leaks(byte):
    """every device block filled with 0xff / 0x55 before it is handed out, red zones round it: the warm-up (W = 61) and the continuing scenario
    compute what the oracle computes, no zone is damaged and nothing is left behind close()"""
    c = P.make_ctx(WA_DEV_POISON=1, WA_DEV_POISON_BYTE=byte, WA_DEV_GUARD=1, WA_DEV_GUARD_BYTE=P.GUARD_BYTE[byte])
    mine = grid_maker(c)
    try:
        for name in ("warmup61", "continuing"):
            check(c, mine, name, off=False, alone=False)
        for dg in mine.made.values():
            dg.close()
        c.trim()
        s = c.guard_stats()
        assert s["live_blocks"] == 0 and s["live_bytes"] == 0 and s["front_damaged"] + s["back_damaged"] == 0 and s["checked"] > 0, s
    finally:
        c.close()
