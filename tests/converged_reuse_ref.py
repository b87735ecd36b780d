"""One solver, more than one search: the scenarios of test_gpu_converged_reuse.py and test_converged_reuse_rules.py, and their play on the C oracle.
No GPU code here.

A scenario is a list of steps on ONE solver (one grid, n_slots, max_colony):
  ("init", p0[, slot])        wa_acs_init_pheromone: in-bounds edges p0, the others 0 (slot -1: every slot)
  ("reset", p0[, slot])       wa_acs_reset_pheromone: every edge p0
  ("begin", {...})            wa_acs_begin: see begin() for the fields; `streams` has one entry per search of the batch (slots 0 .. P-1)
  ("run", k)                  wa_acs_run
  ("read",)                   sync and read everything of the search that is running (it ends here: no run follows before the next begin)
  ("result",)                 result() alone
  ("profile", N)              wa_acs_profile: stamped every Nth generation, 0: off
  ("evaporate", rho, reps)    wa_acs_evaporate on slot 0.  The oracle has no stand-alone evaporation: only directly in front of an init / reset of every
                              slot.  It is there to flip the buffers' parity, not to change a field anyone reads
  ("stragglers", g)           wa_acs_set_stragglers

play() runs the steps on the oracle, one oracle_lib.Acs per slot; a.solve() called again on the same object continues on the field the search before
left, a.reset() is the reset.  The oracle initialises (edges out of bounds 0) only when it is created, so an "init" step takes a new object; nothing
but the field outlives a search in the oracle (best.L starts at infinity), so that is the same thing.

Which generations are replays.  replays(): the trace rows that allow it (the necessary condition of test_gpu_converged_run.py's docstring: every ant
finite, steps == colony * (best_len - 1), iteration best == best == the best before).  is_replay(): the sufficient one, the sequence played again up
to that generation and every ant's path compared with the best path.

Where the windows are.  DESIGN 4p, "Which generations": the host places them without looking at a verdict -- in front of the first generation no
window covers yet, WA_CONVERGED_WINDOW (32) generations, never the last generation of a wa_acs_run call, never a stamped generation, none in a call
of one generation.  windows() restates that; a lone search's window of three generations or more in front of a stamped or last-of-call generation
is judged (it may be carried).  expect() puts the two together: what the oracle's evidence lets a test demand of the counters."""
import collections
import functools

import numpy as np

import oracle_lib as O
import test_gpu_converged_run as R

WINDOW = 32          # WA_CONVERGED_WINDOW's default
BOX = (13, 11, 9)    # nx, ny, nz
BOX_PRECISION = 0.0173

Scenario = collections.namedtuple("Scenario", "grid n_slots max_colony steps")
Search = collections.namedtuple("Search", "index begin gens pieces period stragglers first read want paths field")
# first: ("init" / "reset", p0) when the slot's search starts from such a field, None when it continues on a trained one (or the slot is idle);
# want: what test_gpu_converged_run.collect returns, paths: every ant's path of the last generation; field: the slot's field behind the search, idle or not
Search.__new__.__defaults__ = (None,) * len(Search._fields)


@functools.lru_cache(maxsize=None)
def grid(key):
    """(oracle grid, (start id, end id)).  c2 / c5: the 12^3 grids of test_gpu_converged_run.py; box: 13 x 11 x 9 at precision 0.0173, 3 % occupied"""
    if key in ("c2", "c5"):
        return R.ogrid(12, 0.02 if key == "c2" else 0.05)
    nx, ny, nz = BOX
    free = (np.random.RandomState(2024).uniform(size=nx * ny * nz) >= 0.03).astype(np.uint8)
    p = np.float32(BOX_PRECISION)
    g = O.Grid(np.arange(nx, dtype=np.float32) * p, np.arange(ny, dtype=np.float32) * p, np.arange(nz, dtype=np.float32) * p, free, p, 0)
    ends = g.resolve(g.node_pt(1, 1, 1)), g.resolve(g.node_pt(nz - 2, ny - 2, nx - 2))
    for v in ends:
        g.free[v] = 1
    return g, ends


def begin(case="firm", **kw):
    """a begin step with the colony, rho, generations and seed of R.CASES[case]; kw overrides.  rev: from the grid's end point to its start point;
    mode REF: srand(seed) goes in front of the begin (one slot)"""
    _, _, colony, rho, gens, seed = R.CASES[case]
    b = dict(colony=colony, rho=rho, alpha=1, beta=0.6, pheromone_0=1.0, seed=seed, streams=(0,), mode=O.DEV, max_iteration=gens, rev=False)
    b.update(kw)
    return ("begin", b)


def search(case="firm", run=None, read=True, **kw):
    """begin, run(s), read: the steps of one whole search.  run: generations per call (default: max_iteration in one call)"""
    b = begin(case, **kw)
    runs = [b[1]["max_iteration"]] if run is None else ([run] if isinstance(run, int) else list(run))
    return [b] + [("run", k) for k in runs] + ([("read",)] if read else [])


def windows(pieces, period=0, g0=0, window=WINDOW):
    """[(first generation, length, judged)] of the windows a lone or batched search gets: pieces are the generations per wa_acs_run call"""
    out, until, gen = [], 0, g0

    def at(g, last):
        w = min(window, last - g)
        if period:
            if g % period == 0:
                return 0
            w = min(w, (g // period + 1) * period - g)
        return max(w, 0)
    for k in pieces:
        last = gen + k - 1
        for g in range(gen, gen + k):
            if k > 1 and g >= until:
                w = at(g, last)
                if w >= 1:
                    out.append((g, w, w >= 3 and at(g + w, last) < 1))
                    until = g + w
        gen += k
    return out


def _solve(a, sc, b, gens, rng):
    g, (sid, eid) = grid(sc.grid)
    if b["rev"]:
        sid, eid = eid, sid
    return a.solve(sid, eid, gens, float(b["colony"] / 0.35), fixed_colony=b["colony"], mode=b["mode"], rng=rng, seed=b["seed"], stream=b["stream"],
                   alpha=b["alpha"], beta=b["beta"], rho=b["rho"], pheromone_0=b["pheromone_0"])


def _collect(a, tr):
    lens, L = a.last_ants()
    return dict(steps=tr["steps"], finite=tr["finite"], colony=tr["colony"], bestL=R.bits(tr["bestL"]), iterbestL=R.bits(tr["iterbestL"]),
                cost=R.bits(a.best_L), path=a.best_path()[0], field=R.bits(a.pheromone()), antL=R.bits(L), antLen=lens)


@functools.lru_cache(maxsize=None)
def play(name, slot=0, upto=None):
    """scenario `name` on the oracle as slot `slot` sees it: one Search per begin step (want None where the slot is idle or nothing was run).
    upto = (index, gens): stop behind `gens` generations of search `index` (the searches before it in full) and return that Search alone.
    Computed once and shared: nothing of it is modified later."""
    sc = SCENARIOS[name]
    g, _ = grid(sc.grid)
    a = O.Acs(g)                       # a new solver's field is the init field, 1.0
    out, cur = [], None
    first, period, stragglers = ("init", 1.0), 0, None

    def close():
        nonlocal cur, first
        if cur is None:
            return None
        b, pieces, read, per, strag = cur
        cur = None
        gens = sum(pieces)
        idx = len(out)
        if upto and upto[0] == idx:
            gens = upto[1]
        mine = slot < len(b["streams"])
        want = paths = None
        if mine and gens > 0:
            bb = dict(b, stream=b["streams"][slot])
            tr = _solve(a, sc, bb, gens, O.srand(b["seed"]) if b["mode"] == O.REF else None)
            want, paths = _collect(a, tr), a.last_paths()
        s = Search(idx, b, gens, tuple(pieces), per, strag, first if mine else None, read, want, paths, R.bits(a.pheromone()))
        if mine and gens > 0:
            first = None
        out.append(s)
        return s
    steps = list(sc.steps)
    for i, st in enumerate(steps):
        op = st[0]
        if op in ("init", "reset"):
            close()
            if (st[2] if len(st) > 2 else -1) in (-1, slot):
                if op == "init":
                    a = O.Acs(g, pheromone_0=st[1])
                else:
                    a.reset(st[1])
                first = (op, st[1])
        elif op == "begin":
            close()
            assert len(st[1]["streams"]) <= sc.n_slots and st[1]["colony"] <= sc.max_colony
            cur = [st[1], [], False, period, stragglers]
        elif op == "run":
            assert cur is not None and not cur[2], "a read ends its search"
            cur[1].append(st[1])
        elif op == "read":
            cur[2] = True
        elif op == "profile":
            period = st[1]
            if cur is not None and cur[1]:
                close()                # (between two searches: the one that ran is over)
            elif cur is not None:
                cur[3] = period
        elif op == "evaporate":
            close()
            nxt = steps[i + 1] if i + 1 < len(steps) else ("",)
            assert nxt[0] in ("init", "reset") and (nxt[2] if len(nxt) > 2 else -1) == -1, "the oracle cannot evaporate: an init / reset of every slot follows"
        elif op == "stragglers":
            stragglers = st[1]
            if cur is not None:
                cur[4] = stragglers
        else:
            assert op == "result", op
        if upto and len(out) > upto[0]:
            return out[upto[0]]
    close()
    return out[upto[0]] if upto else out


def replays(name, slot, index):
    """generations of a search whose trace row allows a replay (necessary)"""
    w = play(name, slot)[index].want
    best = w["bestL"].view(np.float32)
    found = np.isfinite(best)
    n_best = np.rint(np.where(found, best, 0) / grid(SCENARIOS[name].grid)[0].precision).astype(np.int64)   # nodes - 1 of a 6-neighbour path of that length
    ok = found & (w["finite"] == w["colony"]) & (w["steps"] == w["colony"] * n_best) & (w["iterbestL"] == w["bestL"])
    ok[1:] &= w["bestL"][1:] == w["bestL"][:-1]
    ok[0] = False
    return [int(v) for v in np.flatnonzero(ok)]


def is_replay(name, slot, index, g):
    """sufficient: the sequence again up to generation g of search `index`; every ant of g walks the best path, and that is the path of generation
    g - 1 (the best path changes only with a strictly smaller cost)"""
    if g < 1:
        return False
    s = play(name, slot, upto=(index, g + 1))
    w = s.want
    return bool(w["bestL"][g] == w["bestL"][g - 1]) and all(np.array_equal(p, w["path"]) for p in s.paths)


@functools.lru_cache(maxsize=None)
def all_replays(name, slot, index):
    """every replay generation of a search, each one confirmed by is_replay (about one oracle search per candidate)"""
    return frozenset(g for g in replays(name, slot, index) if is_replay(name, slot, index, g))


def no_stragglers(s):
    """ants are handed over to the next generation's launch only with alpha == 1 and while the hand-over is on"""
    return s.stragglers == 0 or s.begin["alpha"] != 1


def expect(name, slot, index):
    """What the oracle's trace rows let a test demand of the counters of a search: dict(windows=[(g0, W, judged)], commit=g0 of the last window
    whose first generation is a replay, or None, carried=(g0, W) of the last judged window of a lone search of which every generation, and the one
    behind it, is a replay, or None).  A window does nothing while stragglers are pending, and ants are handed over during the first 64 generations:
    a window in front of generation 65 or earlier counts only where there is no hand-over.  The trace rows are the necessary condition only:
    confirmed() is the sufficient one for exactly the generations used here, and test_converged_reuse_rules.py holds every claim against it."""
    s = play(name, slot)[index]
    rep = set(replays(name, slot, index))
    lone = len(s.begin["streams"]) == 1
    win = windows(s.pieces, s.period) if s.begin["mode"] == O.DEV else []
    free = [(g0, w, j) for g0, w, j in win if s.read and (g0 > 65 or no_stragglers(s))]   # (a search that is not read shows no counters of its own)
    commits = [g0 for g0, w, _ in free if g0 in rep]
    carried = [(g0, w) for g0, w, judged in free if lone and judged and all(t in rep for t in range(g0, g0 + w + 1))]
    return dict(windows=win, commit=commits[-1] if commits else None, carried=carried[-1] if carried else None)


def confirmed(name, slot, index):
    """expect()'s claims hold by the sufficient condition"""
    e = expect(name, slot, index)
    ok = e["commit"] is None or is_replay(name, slot, index, e["commit"])
    if e["carried"]:
        g0, w = e["carried"]
        ok = ok and all(is_replay(name, slot, index, t) for t in range(g0, g0 + w + 1))
    return ok


def exact(name, slot, index):
    """dict(enqueued, whole, cut, generations) of a search without hand-over of stragglers, from all_replays(): a window commits the replays it
    begins with"""
    s = play(name, slot)[index]
    assert no_stragglers(s)
    rep = all_replays(name, slot, index)
    out = dict(enqueued=0, whole=0, cut=0, generations=0)
    for g0, w, _ in windows(s.pieces, s.period):
        j = 0
        while j < w and g0 + j in rep:
            j += 1
        out["enqueued"] += 1
        out["whole"] += j == w
        out["cut"] += 0 < j < w
        out["generations"] += j
    return out


# ------------------------------------------------------------------ the scenarios
def warmup(W):
    """bench.py: init, a throw-away search with seed + 1000 and max_iteration = W, sync, init, the timed search (here firm, stamped every 10th)"""
    return Scenario("c2", 1, 50, [("init", 1.0)] + search("firm", seed=1007, max_iteration=W) + [("init", 1.0), ("profile", 10)] + search("firm"))


def abandoned(case, k, result):
    """begin(max_iteration = 100), run(k) only; then -- without a sync, with or without a result() read -- reset and the next search on another stream"""
    if case == "partial":   # rho 0.9, calls of 70 and 4 (test_gpu_converged_owed.py): window 70-72 commits whole, an ant leaves the path in 73
        return Scenario("c5", 1, 30, [("stragglers", 0)] + search(case, run=k, read=False) + ([("result",)] if result else []) + [("reset", 1.0)]
                        + search(case, streams=(1,)))
    return Scenario("c2", 1, 50, [("profile", 10)] + search(case, run=k, read=False) + ([("result",)] if result else []) + [("reset", 1.0)] + search(case, streams=(1,)))


def continuing(stragglers):
    """firm; on its field the same ends with 20 ants for 80 generations; then the reversed ends with 50 ants.  The continued searches run a call of
    one generation first: a call of several enqueues its first window in front of generation 0, where there is no best path yet, and the next one
    32 generations on; behind a call of one generation the first window stands in front of generation 1.  The second search ends with a call of
    13 generations, so that a window (67-78) stands behind the generations in which ants may be handed over and its commit can be demanded with the
    hand-over on too"""
    st = [] if stragglers is None else [("stragglers", stragglers)]
    return Scenario("c2", 1, 50, st + search("firm") + search("small", run=(1, 66, 13)) + search("firm", rev=True, run=(1, 99)))


SCENARIOS = {}
for _W in (5, 40, 61, 100):
    SCENARIOS["warmup%d" % _W] = warmup(_W)
for _k in (26, 34, 60, 61):
    SCENARIOS["abandoned%d" % _k] = abandoned("firm", _k, False)
    SCENARIOS["abandoned%d_result" % _k] = abandoned("firm", _k, True)
SCENARIOS["abandoned73"] = abandoned("partial", (70, 4), False)
SCENARIOS["abandoned73_result"] = abandoned("partial", (70, 4), True)
SCENARIOS["continuing"] = continuing(None)
SCENARIOS["continuing_no_stragglers"] = continuing(0)
SCENARIOS["continuing_partial"] = Scenario("c5", 1, 30, [("stragglers", 0)] + search("partial") + search("partial", seed=5, max_iteration=60, run=(1, 59)))
# DEV, reset, REF, reset, DEV on stream 1; then init and the same search again: that one is held against R.ref("firm", 1) too, the whole field
# included (R.ref starts from an init field, whose edges out of bounds are 0 where a reset field has p0)
SCENARIOS["modes"] = Scenario("c2", 1, 50, search("firm") + [("reset", 1.0)] + search("firm", mode=O.REF) + [("reset", 1.0)] + search("firm", streams=(1,))
                              + [("init", 1.0)] + search("firm", streams=(1,)))
# searches whose window counters are held against exact(): every candidate generation played again, about a second each
EXACT = {("continuing_no_stragglers", 1), ("continuing_no_stragglers", 2), ("continuing_partial", 1), ("par_alpha0", 0), ("par_alpha2", 0), ("par_alpha3_beta03_stamped", 0)}
for _n in (99, 100):
    SCENARIOS["lone%d" % _n] = Scenario("c2", 3, 50, search("firm", max_iteration=_n) + [("reset", 1.0, 0)] + search("firm", streams=(0, 1, 2)) + search("firm", run=(1, 99)))
# (small in calls of 67 and 13 generations: its last window, 67-78, stands behind the generations in which ants may be handed over)
SCENARIOS["colony_and_rho"] = Scenario("c2", 1, 64, search("wide") + [("reset", 1.0)] + search("small", run=(67, 13)) + [("reset", 1.0)] + search("firm")
                                       + search("firm", rho=0.9, run=(1, 99)))
SCENARIOS["profiling"] = Scenario("c2", 1, 50, [("profile", 10)] + search("firm") + [("profile", 0), ("evaporate", 0.5, 1), ("reset", 1.0)] + search("firm", streams=(1,))
                                  + [("evaporate", 0.5, 3), ("reset", 1.0), ("profile", 5)] + search("firm", streams=(2,)))

# single searches on a fresh solver: name -> (grid, begin fields, p0 of the init in front)
PARAMETERS = {
    "plain": ("c2", dict(), 1.0),
    "alpha2": ("c2", dict(alpha=2), 1.0),
    "alpha3_beta03": ("c2", dict(alpha=3, beta=0.3), 1.0),
    "rho05_beta09": ("c2", dict(rho=0.5, beta=0.9), 1.0),
    "p0_025": ("c2", dict(pheromone_0=0.25), 0.25),
    "box": ("box", dict(), 1.0),
    "alpha0": ("c2", dict(alpha=0), 1.0),
}
for _name, (_g, _kw, _p0) in PARAMETERS.items():
    SCENARIOS["par_" + _name] = Scenario(_g, 1, 50, [("init", _p0)] + search("firm", **_kw))
    if _kw.get("alpha", 1) != 1:
        SCENARIOS["par_" + _name + "_stamped"] = Scenario(_g, 1, 50, [("init", _p0), ("profile", 10)] + search("firm", **_kw))
