"""tests/stops_ref.py, the numpy restatement of the weld passes in a timed trajectory (include/weldacs.h rules 40 - 42), held against facts
that do not come from it: a trajectory with stops is the concatenation of its pieces timed alone by retime_ref.retime; a tick inside a
dwell is the stop's sample; without a stop the calls are their parents; a dwell sized by axes_dwells gives the turn its time.  No GPU."""
import numpy as np
import pytest

import retime_ref as R
import stops_ref as S
import ticks_ref as K
import torch_ref as T

Q = R.Q


def random_pieces(rs, n_stops, first_single=False, last_single=False):
    """n_stops + 1 pieces of 2 - 60 samples, each beginning where the one before ends; a piece of one sample at either end on request"""
    pieces, at = [], rs.uniform(-2.0, 2.0, 3)
    for k in range(n_stops + 1):
        m = int(rs.randint(2, 61))
        if (k == 0 and first_single) or (k == n_stops and last_single):
            m = 1
        steps = rs.uniform(-0.3, 0.3, (m - 1, 3))
        p = np.concatenate([[at], at + np.cumsum(steps, 0)]).astype(np.float32)
        if pieces:
            p[0] = pieces[-1][-1]
        pieces.append(p)
        at = p[-1].astype(np.float64)
    return pieces


def split_cases():
    """40 cases: (seed, stops, a stop at segment 0, a stop at segment n - 2, two stops in a row at the first joint)"""
    cases = []
    for seed in range(40):
        cases.append((seed, 1 + seed % 4, seed % 5 == 1, seed % 5 == 2, seed % 5 == 3))
    return cases


@pytest.mark.parametrize("seed,n_stops,first,last,twice", split_cases())
def test_split_identity(seed, n_stops, first, last, twice):
    rs = np.random.RandomState(1000 + seed)
    pieces = random_pieces(rs, n_stops, first, last)
    dwells = [float(d) for d in rs.choice([0.0, 0.003, 0.05, 0.7], n_stops)]
    if twice:
        dwells[0] = [dwells[0], 0.02]
    lim = R.limits(v_max=rs.uniform(0.5, 2.0), acc=rs.uniform(0.5, 4.0), dec=rs.uniform(0.5, 4.0), a_lat=rs.uniform(0.2, 2.0))
    xyz, dwell, at = S.with_stops(pieces, dwells)
    n = len(xyz)
    if first:
        assert at[0] == 0
    if last:
        assert at[-1] == n - 2
    v_limit = rs.uniform(0.2, 3.0, n).astype(np.float32) if seed % 2 else None
    whole = S.retime_stops(xyz, lim, dwell, v_limit=v_limit, tick=0.01)
    assert whole["stops"] == dict(n_stops=len(at), n_stop_samples=len(set(at) | set(a + 1 for a in at)),
                                  dwell_q=int(sum(int(np.rint(np.float64(d) * R.QF)) for d in np.concatenate([np.atleast_1d(d) for d in dwells]))))
    # the pieces alone: sample ranges between the stops (a doubled sample between two stops in a row is a piece of one sample)
    starts = [0] + [a + 1 for a in at]
    ends = [a + 1 for a in at] + [n]
    w_q, time_q, bound, offset = [], [], [], 0
    for k, (s, e) in enumerate(zip(starts, ends)):
        if e - s >= 2:
            r = R.retime(xyz[s:e], lim, None if v_limit is None else v_limit[s:e], None, 0.01, want_ticks=False)
            w, t, b = r["w_q"], r["time_q"], r["bound"]
        else:
            w, t, b = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.uint8)
        w_q.append(w)
        time_q.append(t + offset)
        bound.append(b)
        offset += int(t[-1])
        if k < len(at):
            offset += int(whole["dq"][at[k]])
    assert np.array_equal(whole["w_q"], np.concatenate(w_q))
    assert np.array_equal(whole["time_q"], np.concatenate(time_q))
    away = np.ones(n, bool)
    for a in at:
        away[a] = away[a + 1] = False
    assert np.array_equal(whole["bound"][away], np.concatenate(bound)[away])
    assert (whole["bound"][~away] >> 4 == R.KIND_END).all() and (whole["w_q"][~away] == 0).all()
    assert whole["summary"]["time_q"] == offset and whole["summary"]["n_bound"][0] == 2 + int((~away[1:-1]).sum())
    # the recurrences of rule 3, one sample after the other, agree with the closed forms at the reset caps
    F, B = R.passes_sequential(whole["C"], whole["A"], whole["D"])
    assert np.array_equal(B, whole["w_q"]) and np.array_equal(F, whole["F"])


def dwell_scene(dwell_ticks, tick=0.01):
    a = R.densify([[0, 0, 0], [1, 0, 0]], 40)
    b = R.densify([[1, 0, 0], [1, 1, 0]], 30)
    xyz, dwell, at = S.with_stops([a, b], [dwell_ticks * tick])
    return xyz, dwell, at[0]


@pytest.mark.parametrize("dwell_ticks", [0.0, 0.3, 5.0, 12.345, 300.0])
def test_dwell_ticks_are_the_stop_sample(dwell_ticks):
    tick = 0.01
    xyz, dwell, s = dwell_scene(dwell_ticks, tick)
    lim = R.limits(v_max=2, acc=3, dec=5)
    r = S.retime_stops(xyz, lim, dwell, tick=tick)
    tq, t0, t1 = r["tick_q"], int(r["time_q"][s]), int(r["time_q"][s + 1])
    assert t1 - t0 == r["dq"][s] == int(np.rint(np.float64(dwell_ticks * tick) * R.QF))
    # ticks k * tq with t0 <= k * tq < t1, counted in integers
    first, beyond = -(-t0 // tq), -(-t1 // tq)
    inside = np.arange(first, beyond)
    _, i, _, _, dw = S.dwell_ticks(xyz, r["time_q"], r["w_q"], lim["acc"], lim["dec"], tq)
    assert np.array_equal(np.flatnonzero(dw), inside) and (i[dw] == s).all()
    assert len(inside) in (int((t1 - t0) // tq), int((t1 - t0) // tq) + 1)
    assert np.array_equal(r["ticks"][inside].view(np.uint32), np.repeat(xyz[s:s + 1], len(inside), 0).view(np.uint32))
    if dwell_ticks == 0.3:
        assert len(inside) <= 1
    if dwell_ticks == 0.0:
        assert len(inside) == 0


def test_null_dwell_is_retime():
    grid, xyz, lim, v_limit, tick = R.random_scene(3)
    a, b = S.retime_stops(xyz, lim, None, v_limit, grid, tick), R.retime(xyz, lim, v_limit, grid, tick)
    assert a.pop("stops") == dict(n_stops=0, n_stop_samples=0, dwell_q=0)
    assert a.keys() == b.keys()
    for k in b:
        assert np.array_equal(a[k], b[k]) if isinstance(b[k], np.ndarray) else a[k] == b[k], k
    # and a dwell array without a stop changes nothing either
    c = S.retime_stops(xyz, lim, np.full(len(xyz) - 1, -1.0), v_limit, grid, tick)
    for k in ("time_q", "w_q", "bound", "ticks"):
        assert np.array_equal(c[k], b[k]), k
    assert c["summary"] == b["summary"]


def test_tick_reduction_without_a_dwell():
    grid, xyz, q, tool = K.slab_turn_scene()
    xyz = np.concatenate([xyz[:50], xyz[49:]])   # (a doubled sample WITHOUT a duration is no dwell)
    q = np.concatenate([q[:50], q[49:]])
    lim = R.limits(v_max=3, acc=4, dec=6)
    r = R.retime(xyz, lim, tick=0.01)
    a = S.tick_axes_stops(xyz, q, r["time_q"], r["w_q"], lim["acc"], lim["dec"], 0.01, grid, tool, 2)
    b = K.tick_axes(xyz, q, r["time_q"], r["w_q"], lim["acc"], lim["dec"], 0.01, grid, tool, 2)
    assert a["stops"] == dict(n_dwell_ticks=0, n_tagged=0, max_dwell_turn=0) and a["tag"] is None and not a["dwell"].any()
    assert a["summary"] == b["summary"]
    for k in ("axes", "qt", "blocked", "pos"):
        assert np.array_equal(a[k], b[k]), k


def turning_stop(qa, qb, dwell_ticks=20, tick=0.01):
    xyz, dwell, s = dwell_scene(dwell_ticks, tick)
    q = np.where((np.arange(len(xyz)) <= s)[:, None], np.asarray(qa), np.asarray(qb)).astype(np.int64)
    lim = R.limits(v_max=2, acc=3, dec=5)
    r = S.retime_stops(xyz, lim, dwell, tick=tick)
    return xyz, q, s, lim, r


def test_axes_during_a_dwell():
    qa, qb = T.quantise_all(np.array([[1.0, 0.2, 0.0], [-0.3, 1.0, 0.4]]))
    xyz, q, s, lim, r = turning_stop(qa, qb, dwell_ticks=20.5)
    tags = np.zeros(len(xyz) - 1, np.uint8)
    tags[s] = 7
    tags[s + 1:] = 1
    o = S.tick_axes_stops(xyz, q, r["time_q"], r["w_q"], lim["acc"], lim["dec"], 0.01, seg_tag=tags)
    k = np.flatnonzero(o["dwell"])
    assert len(k) >= 20 and o["stops"]["n_dwell_ticks"] == len(k)
    # the axes differ only across the stop: before the dwell every tick has the first axis, behind it the second (each as rule 1
    # gives it back: quantising a quantised triple again can move a component by 1)
    qa_r, qb_r = K.quantise_rows(np.array([qa, qb], np.float64))
    assert (o["qt"][:k[0]] == qa_r).all() and (o["qt"][k[-1] + 1:] == qb_r).all()
    chord = ((o["qt"][k].astype(np.int64) - qb) ** 2).sum(1)
    assert (np.diff(chord) <= 0).all() and chord[0] > chord[-1]
    assert (o["tag"][k] == 7).all() and (o["tag"][:k[0]] == 0).all() and (o["tag"][k[-1] + 1:] == 1).all()
    assert o["stops"]["n_tagged"] == int((o["tag"] != 0).sum()) == len(o["tag"]) - k[0]
    turn = T.turn(o["qt"][:-1], o["qt"][1:])
    assert o["stops"]["max_dwell_turn"] == int(turn[k - 1].max()) > 0
    assert o["summary"]["max_tick_turn"] >= o["stops"]["max_dwell_turn"]
    assert np.array_equal(o["pos"][k].view(np.uint32), np.repeat(xyz[s:s + 1], len(k), 0).view(np.uint32))


def test_a_dwell_that_starts_on_a_tick_starts_on_the_first_axis():
    qa, qb = np.array([16384, 0, 0]), np.array([0, 16384, 0])
    xyz, dwell, s = dwell_scene(10)
    q = np.where((np.arange(len(xyz)) <= s)[:, None], qa, qb).astype(np.int64)
    n = len(xyz)
    tq = int(np.rint(0.01 * R.QF))
    # times made by hand: the stop begins at tick 30 exactly and lasts 10 ticks
    time_q = np.concatenate([np.linspace(0, 30 * tq, s + 1).astype(np.int64), 40 * tq + np.linspace(0, 25 * tq, n - s - 1).astype(np.int64)])
    w_q = np.zeros(n, np.int64)
    o = S.tick_axes_stops(xyz, q, time_q, w_q, 3.0, 5.0, 0.01)
    k = np.flatnonzero(o["dwell"])
    assert k.tolist() == list(range(30, 40))
    assert np.array_equal(o["qt"][30], qa) and np.array_equal(o["qt"][40], qb)
    assert np.array_equal(o["qt"][35], K.quantise_rows(np.array([[0.5, 0.5, 0.0]]))[0])


def test_opposite_axes_give_the_first_axis_where_they_cancel():
    qa = np.array([16384, 0, 0])
    xyz, dwell, s = dwell_scene(10)
    q = np.where((np.arange(len(xyz)) <= s)[:, None], qa, -qa).astype(np.int64)
    n = len(xyz)
    tq = int(np.rint(0.01 * R.QF))
    time_q = np.concatenate([np.linspace(0, 30 * tq, s + 1).astype(np.int64), 40 * tq + np.linspace(0, 25 * tq, n - s - 1).astype(np.int64)])
    o = S.tick_axes_stops(xyz, q, time_q, np.zeros(n, np.int64), 3.0, 5.0, 0.01)
    assert o["lam"][35] == 0.5 and np.array_equal(o["qt"][35], qa)    # the interpolant is all zero: q_i
    assert np.array_equal(o["qt"][34], qa) and np.array_equal(o["qt"][36], -qa)


def test_axes_dwells_give_the_turn_its_time():
    rs = np.random.RandomState(5)
    pieces = random_pieces(rs, 4)
    xyz, dwell, at = S.with_stops(pieces, [0.0, [5.0, 0.0], 0.001, 2.0])
    n = len(xyz)
    dirs = T.quantise_all(T.fib_dirs(8, 1.2, (0.0, 0.0, 1.0)))
    piece_of = np.searchsorted(np.asarray(at), np.arange(n), side="left")
    q = dirs[piece_of % 8]
    q[at[-1] + 1:] = q[at[-1]]    # (the last joint keeps its axis: a stop without a turn)
    omega = 1.5
    d = S.axes_dwells(xyz, q, omega, dwell)
    jump = (d["L"] == 0) & (d["D"] > 0)
    assert d["summary"]["n_jump"] == int(jump.sum()) >= 3 and d["summary"]["n_stops"] == len(at)
    assert 0 < d["summary"]["n_raised"] < d["summary"]["n_jump"]     # 5 s is enough for any turn at this rate (a chord is at most 2), 0 s for none
    assert d["summary"]["max_need"] == float((d["psi"][jump] / omega).max())
    assert (d["dwell"][d["L"] > 0] == -1).all() and (d["dwell"] >= dwell).all()
    r = S.retime_stops(xyz, R.limits(v_max=1.0, acc=2.0, dec=2.0), d["dwell"], tick=0.01)
    need_q = np.floor(d["psi"] / np.float64(omega) * R.QF).astype(np.int64)
    assert (r["T"][jump] >= need_q[jump]).all()
    # without dwell_in: a stop exactly where the axes jump
    d0 = S.axes_dwells(xyz, q, omega)
    assert np.array_equal(d0["dwell"] >= 0, jump) and d0["summary"]["n_raised"] == d0["summary"]["n_jump"] == d0["summary"]["n_stops"]


def test_what_is_refused():
    xyz, dwell, s = dwell_scene(5)
    lim = R.limits(v_max=2, acc=3, dec=5)
    n = len(xyz)
    q = np.tile([0, 0, 16384], (n, 1))
    for bad in (np.nan, np.inf, -np.inf, float(1 << 31)):
        d = dwell.copy()
        d[s] = bad
        with pytest.raises(ValueError):
            S.retime_stops(xyz, lim, d)
    d = dwell.copy()
    d[s] = float(1 << 30)            # 2^60 quanta: accepted
    assert S.retime_stops(xyz, lim, d, want_ticks=False)["stops"]["dwell_q"] == 1 << 60
    d = dwell.copy()
    d[3] = 0.0                         # a stop on a segment that has a length
    with pytest.raises(ValueError):
        S.retime_stops(xyz, lim, d)
    with pytest.raises(ValueError):
        S.axes_dwells(xyz, q, 1.0, d)
    for bad in (np.nan, np.inf):
        d = dwell.copy()
        d[s] = bad
        with pytest.raises(ValueError):
            S.axes_dwells(xyz, q, 1.0, d)
    for omega in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            S.axes_dwells(xyz, q, omega, dwell)
