"""numpy restatement of the weld passes in a timed trajectory (include/weldacs.h rules 40 - 42: wa_traj_retime_stops,
wa_traj_tick_axes_stops, wa_traj_axes_dwells), assembled from the functions of retime_ref (rules 1 - 6 of the retime section) and ticks_ref
(rules 25 and 26) by import: what a stop adds is stated here, everything else is theirs.  No GPU, no product code.

A stop is a segment without length (L_i = 0) that has a duration dq_i = rint(dwell[i] * Q) >= 0.  Both of its samples get a kind-0 cap of
0; its time is T_i = dq_i; rule 6 is unchanged.  A tick inside a dwell stays at p_i while its axis turns from q_i to q_(i+1), linear in
time."""
import numpy as np

import retime_ref as R
import ticks_ref as K

Q = R.Q
QF = R.QF
CAP = R.CAP_INF
STOPS_FIELDS = ("n_stops", "n_stop_samples", "dwell_q")
TICK_STOPS_FIELDS = ("n_dwell_ticks", "n_tagged", "max_dwell_turn")
DWELLS_FIELDS = ("n", "n_jump", "n_stops", "n_raised", "max_need")


def _big_sum(s):
    return sum(int(x) for x in s[s >= (1 << 40)]) + int(s[s < (1 << 40)].sum())


def dwell_quanta(dwell, n):
    """dq int64[n-1], -1 where the segment is no stop; ValueError for an entry that is not finite or reaches 2^61 quanta"""
    dwell = np.asarray(dwell, np.float64).reshape(-1)
    if len(dwell) != n - 1 or not np.isfinite(dwell).all():
        raise ValueError("dwell")
    dq = np.rint(np.where(dwell < 0, 0.0, dwell) * QF)
    if not (dq < float(CAP)).all():
        raise ValueError("dwell reaches 2^61")
    return np.where(dwell < 0, -1, dq.astype(np.int64)).astype(np.int64)


def retime_stops(xyz, lim, dwell=None, v_limit=None, grid=None, tick=0.01, want_ticks=True):
    """wa_traj_retime_stops: retime_ref.retime's dictionary plus "stops"; ValueError where the call answers WA_ERR_ARG"""
    base = R.retime(xyz, lim, v_limit, grid, tick, want_ticks and dwell is None)   # (the arguments, and everything a stop leaves alone)
    if dwell is None:
        return dict(base, stops=dict(n_stops=0, n_stop_samples=0, dwell_q=0))
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    dq = dwell_quanta(dwell, n)
    stop = dq >= 0
    ds, L, A, D = base["ds"], base["L"], base["A"], base["D"]
    if (stop & (L > 0)).any():
        raise ValueError("a stop on a segment that has a length")
    at_stop = np.zeros(n, bool)
    at_stop[:-1] |= stop
    at_stop[1:] |= stop
    C = np.where(at_stop, 0, base["C"]).astype(np.int64)
    kind = np.where(at_stop, R.KIND_END, base["kind"]).astype(np.uint8)
    F, B = R.passes(C, A, D)
    bound = R.bound_bits(C, B, A, D, kind)
    dt, T, tri, t_up = R.times(ds, L, B, lim["acc"], lim["dec"])
    T = np.where(stop, dq, T).astype(np.int64)
    if _big_sum(T) >= CAP:
        raise ValueError("duration reaches 2^61")
    time_q = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    time = int(time_q[-1])
    tick_q = base["tick_q"]
    n_ticks = R.tick_count(time, tick_q)
    summary = dict(n=n, n_ticks=n_ticks, length_q=int(L.sum()), time_q=time,
                   n_bound=[int((kind == k).sum()) for k in range(4)],
                   n_on_cap=int((bound & 1).astype(bool).sum()), n_on_ramp=int((bound & 6).astype(bool).sum()),
                   n_triangle=int(tri.sum()), n_outside=base["summary"]["n_outside"], peak_w_q=int(B.max()))
    out = dict(base, time_q=time_q, w_q=B, bound=bound, summary=summary, C=C, F=F, kind=kind, T=T, dq=dq, ticks=None,
               stops=dict(n_stops=int(stop.sum()), n_stop_samples=int(at_stop.sum()), dwell_q=int(dq[stop].sum())))
    if want_ticks and n_ticks <= R.MAX_TICKS:
        out["ticks"] = R.ticks(xyz, ds, L, B, dt, tri, t_up, time_q, tick_q, lim["acc"], lim["dec"])
    return out


def dwell_ticks(xyz, time_q, w_q, acc, dec, tick_q):
    """rule 6 per tick and rule 41 (a): (taus, segment i, lambda for the AXIS, positions float32, dwell mask)"""
    time_q = np.asarray(time_q, np.int64)
    taus, i, lam, pos = K.tick_params(xyz, time_q, w_q, acc, dec, tick_q)
    L = R._quanta(R.seg_lengths(xyz))
    t0, t1 = time_q[i], time_q[i + 1]
    dw = (L[i] == 0) & (t1 > t0) & (taus < t1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ld = (taus - t0).astype(np.float64) / (t1 - t0).astype(np.float64)
    ld = np.where(ld < 0.0, 0.0, np.where(ld > 1.0, 1.0, ld))
    return taus, i, np.where(dw, ld, lam), pos, dw


def tick_axes_stops(xyz, q, time_q, w_q, acc, dec, tick, grid=None, tool=None, near_add=-1, seg_tag=None):
    """wa_traj_tick_axes_stops: ticks_ref.tick_axes's dictionary plus tag (uint8[n_ticks] or None), dwell (mask) and "stops"."""
    base = K.tick_axes(xyz, q, time_q, w_q, acc, dec, tick, grid, tool, near_add)   # (the arguments; the result where nothing dwells)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    q = K.check_axes(q, n)
    tick_q = int(np.rint(np.float64(tick) * QF))
    _, i, lam, pos, dw = dwell_ticks(xyz, time_q, w_q, acc, dec, tick_q)
    out = base
    if dw.any():
        qa, qb = q[i].astype(np.float64), q[i + 1].astype(np.float64)
        v = qa + (qb - qa) * lam[:, None]
        zero = (v == 0).all(1)
        qt = q[i].copy()
        qt[~zero] = K.quantise_rows(v[~zero])
        k = len(i)
        blocked, near = np.zeros(k, bool), np.zeros(k, np.int64)
        if grid is not None:
            vox, _ = K.T.sample_voxels(grid, pos)
            blocked, near = K.blocked_at(grid, vox, qt, tool, near_add)
        turn = K.T.turn(qt[:-1], qt[1:])
        summary = dict(base["summary"], n_blocked=int(blocked.sum()), first_blocked=int(np.flatnonzero(blocked)[0]) if blocked.any() else -1,
                       n_near=int((~blocked & (near > 0)).sum()), max_tick_turn=int(turn.max()) if len(turn) else 0)
        out = dict(base, axes=(qt.astype(np.float64) / 16384.0).astype(np.float32), qt=qt, blocked=blocked.astype(np.uint8), summary=summary, lam=lam)
    qt = out["qt"]
    turn = np.concatenate([[0], K.T.turn(qt[:-1], qt[1:])])
    tag = None
    if seg_tag is not None:
        seg_tag = np.asarray(seg_tag, np.uint8).reshape(-1)
        if len(seg_tag) != n - 1:
            raise ValueError("seg_tag")
        tag = seg_tag[i]
    stops = dict(n_dwell_ticks=int(dw.sum()), n_tagged=int((tag != 0).sum()) if tag is not None else 0,
                 max_dwell_turn=int(turn[dw].max()) if dw.any() else 0)
    return dict(out, tag=tag, dwell=dw, stops=stops)


def axes_dwells(xyz, q, omega, dwell_in=None):
    """wa_traj_axes_dwells: dict(dwell float64[n-1], summary, need, psi, D, L)"""
    r = K.limits(xyz, q, omega, 1.0, 1.0)   # (the arguments; D, psi and L of rule 25)
    D, psi, L = r["D"], r["psi"], r["L"]
    m = len(D)
    given = np.full(m, -1.0) if dwell_in is None else np.asarray(dwell_in, np.float64).reshape(-1)
    if len(given) != m or not np.isfinite(given).all():
        raise ValueError("dwell_in")
    if ((L > 0) & (given >= 0)).any():
        raise ValueError("a dwell on a segment that has a length")
    jump = (L == 0) & (D > 0)
    need = np.where(jump, psi / np.float64(omega), 0.0)
    raised = jump & (given < need)
    out = np.where(L > 0, -1.0, np.where(jump, np.where(raised, need, given), np.where(given >= 0, given, -1.0)))
    summary = dict(n=len(D) + 1, n_jump=int(jump.sum()), n_stops=int((out >= 0).sum()), n_raised=int(raised.sum()),
                   max_need=float(need.max()) if jump.any() else 0.0)
    return dict(dwell=out, summary=summary, need=need, psi=psi, D=D, L=L)


# ------------------------------------------------------------------ scenes for the tests
def with_stops(pieces, dwells):
    """pieces of a polyline joined by stops.  Piece k + 1 begins at the very sample piece k ends with, so the joint is a segment without
    length: the stop, dwells[k] seconds long.  A list of dwells at a joint repeats the sample once more per further entry (stops in a
    row); a piece of one sample puts a stop at the very start or end.  Returns (xyz float32, dwell float64[n-1], the stop segments)."""
    parts, dwell, at = [], [], []
    n = 0
    for k, p in enumerate(pieces):
        p = np.asarray(p, np.float32).reshape(-1, 3)
        if k > 0:
            assert np.array_equal(p[0], parts[-1][-1])
            ds = np.atleast_1d(dwells[k - 1])
            for d in ds[:-1]:
                parts.append(p[:1])
                at.append(n - 1)
                dwell.append(float(d))
                n += 1
            at.append(n - 1)
            dwell.append(float(ds[-1]))
        parts.append(p)
        dwell += [-1.0] * (len(p) - 1)
        n += len(p)
    return np.concatenate(parts).astype(np.float32), np.asarray(dwell, np.float64), at
