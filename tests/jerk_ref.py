"""numpy restatement of the jerk-limited controller ticks (include/weldacs.h rules 48 - 55: wa_traj_retime_jerk, wa_traj_jerk_window),
assembled from retime_ref (retime rules 1 - 6), stops_ref (rule 40) and ticks_ref (rule 6 per tick) by import: what the moving average
along the arc length adds is stated here, everything else is theirs.  No GPU, no product code.

W ticks are averaged, not in x, y and z but in the arc length: U_k is the arc length of the unfiltered tick k, S_k = floor(mean of the
last W of them), and the output tick is the point of the polyline at arc length S_k.  Two repairs make the result keep what the
unfiltered profile promised: the caps of kinds 1 - 3 are lowered to their minimum over the distance a window can span (R_q) before the
profile is computed, and every dwell is extended by the W - 1 ticks the window eats.

`lower=False` is a switch for the tests alone: it sets R_q = 0, which skips the lowering."""
import bisect

import numpy as np

import retime_ref as R
import stops_ref as S
import ticks_ref as K

Q = R.Q
QF = R.QF
CAP = R.CAP_INF
MAX_W = 1 << 20
LOWERED = 0x40
JERK_FIELDS = ("window", "reach_q", "n_lowered", "n_in", "n_ticks", "max_d1", "max_d2", "max_d3", "in_max_d2", "n_rest_ticks",
               "n_short_rests", "n_back")


def jerk_window(acc, dec, jerk, tick):
    """wa_traj_jerk_window: W = max(1, ceil((2 * max(acc, dec)) / (jerk * tick)))"""
    v = [np.float64(x) for x in (acc, dec, jerk, tick)]
    if not all(np.isfinite(x) and x > 0 for x in v):
        raise ValueError("arguments")
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        w = np.ceil((np.float64(2.0) * max(v[0], v[1])) / (v[2] * v[3]))
    if not w <= float(MAX_W):
        raise ValueError("window above 2^20")
    return max(1, int(w))


def caps13(xyz, lim, v_limit=None, grid=None):
    """rule 2 over kinds 1 - 3 only, for EVERY sample: (C13 int64, kind uint8).  retime_ref.caps on the samples with each end doubled:
    a doubled end has no curvature (u or v is zero) and is no end point, so it keeps its kind-1 / kind-3 cap; the two added samples go."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pad = np.concatenate([xyz[:1], xyz, xyz[-1:]])
    vl = None if v_limit is None else np.concatenate([v_limit[:1], v_limit, v_limit[-1:]]).astype(np.float32)
    C, kind, _ = R.caps(pad, lim, vl, grid)
    return C[1:-1].copy(), kind[1:-1].copy()


def range_min(key, lo, hi):
    """min(key[lo[j] .. hi[j]]) per j by a sparse table of power-of-two minima (the device's way); key uint64"""
    n = len(key)
    width = hi - lo + 1
    levels = [key]
    while (1 << len(levels)) <= int(width.max()):
        h = 1 << (len(levels) - 1)
        prev = levels[-1]
        levels.append(np.minimum(prev, prev[np.minimum(np.arange(n) + h, n - 1)]))
    p = np.floor(np.log2(width)).astype(np.int64)
    p = np.where((np.int64(1) << p) > width, p - 1, p)
    out = np.empty(len(lo), np.uint64)
    for l in range(len(levels)):
        m = p == l
        out[m] = np.minimum(levels[l][lo[m]], levels[l][hi[m] - (1 << l) + 1])
    return out


def lowered_caps(C13, kind13, GL, R_q):
    """rule 49: (C', kind') -- the minimum of C13 over every sample m with GL_max(j-1,0) - R_q <= GL_m <= GL_min(j+1,n-1) + R_q, its kind
    the lowest-numbered one among the samples attaining it.  R_q = 0: nothing is lowered."""
    if R_q == 0:
        return C13.copy(), kind13.copy()
    n = len(C13)
    j = np.arange(n)
    lo = np.searchsorted(GL, GL[np.maximum(j - 1, 0)] - R_q, side="left")
    hi = np.searchsorted(GL, GL[np.minimum(j + 1, n - 1)] + R_q, side="right") - 1
    key = C13.astype(np.uint64) * np.uint64(4) + kind13.astype(np.uint64)
    m = range_min(key, lo, hi)
    return (m >> np.uint64(2)).astype(np.int64), (m & np.uint64(3)).astype(np.uint8)


def arcs(xyz, L, GL, time_q, B, acc, dec, tick_q):
    """rule 52: U int64[n_u], the arc length of every unfiltered tick"""
    _, i, lam, _ = K.tick_params(xyz, time_q, B, acc, dec, tick_q)
    return GL[i] + np.rint(lam * L[i].astype(np.float64)).astype(np.int64)


def window_means(U, W, length_q):
    """rule 53: S_k = floor((U_k + ... + U_(k-W+1)) / W) for k = 0 .. n_u + W - 2, U = 0 in front and length_q behind; the window sums
    are differences of prefix sums modulo 2^64 (exact, since W * length_q < 2^62).  The prefix array is uint64 from its first element:
    a Python 0 in front makes numpy promote the whole array to float64, which drops the low bits of every sum above 2^53."""
    n_u = len(U)
    with np.errstate(over="ignore"):
        P = np.concatenate([np.zeros(1, np.uint64), np.cumsum(U.astype(np.uint64), dtype=np.uint64)])
        k = np.arange(n_u + W - 1, dtype=np.int64)
        s = P[np.minimum(k, n_u - 1) + 1] - P[np.maximum(k - W + 1, 0)] + (np.maximum(k - n_u + 1, 0) * np.int64(length_q)).astype(np.uint64)
    return (s // np.uint64(W)).astype(np.int64)


def locate(S_q, GL, L, stop):
    """rule 54: (segment i, rest mask, at_end mask) per filtered tick"""
    n = len(GL)
    nxt = np.full(n + 1, n, np.int64)   # the lowest stop segment at or after a sample
    for i in range(n - 2, -1, -1):
        nxt[i] = i if stop[i] else nxt[i + 1]
    lo = np.searchsorted(GL, S_q, side="left")
    first = nxt[lo]
    rest = (first < n - 1) & (GL[np.minimum(first, n - 1)] == S_q)
    i = np.minimum(np.searchsorted(GL, S_q, side="right") - 1, n - 2)
    at_end = ~rest & (S_q >= GL[i + 1])
    return np.where(rest, first, i), rest, at_end


def positions(xyz, S_q, GL, L, i, rest, at_end):
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    still = rest | (~at_end & (L[i] == 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (S_q - GL[i]).astype(np.float64) / L[i].astype(np.float64)
    lam = np.where(still | at_end, 0.0, lam)
    out = (p[i] + (p[i + 1] - p[i]) * lam[:, None]).astype(np.float32)
    out[still] = p32[i[still]]
    out[at_end] = p32[i[at_end] + 1]
    return out


def _absmax(d):
    return max((abs(int(x)) for x in (d.min(), d.max())), default=0) if len(d) else 0


def summary_of(S_q, U, W, length_q, R_q, n_lowered, rest, first, GL, stop, dq, tick_q):
    n_u = len(U)
    pad = np.concatenate([np.zeros(W + 1, np.int64), U, np.full(W + 2, length_q, np.int64)])   # k = -W - 1 .. n_u + W + 1
    short = 0
    if stop.any():
        heads = {}
        for i in np.flatnonzero(stop):   # the groups: stops that share one GL; the lowest-numbered one takes the rest ticks
            heads.setdefault(int(GL[i]), [int(i), 0])[1] += int(dq[i])
        got = np.bincount(first[rest], minlength=len(GL))
        short = sum(1 for h, need in heads.values() if int(got[h]) < need // tick_q)
    d1 = np.diff(S_q)
    return dict(window=W, reach_q=R_q, n_lowered=int(n_lowered), n_in=n_u, n_ticks=len(S_q), max_d1=_absmax(d1),
                max_d2=_absmax(np.diff(S_q, 2)), max_d3=_absmax(np.diff(S_q, 3)), in_max_d2=_absmax(np.diff(pad, 2)),
                n_rest_ticks=int(rest.sum()), n_short_rests=short, n_back=int((d1 < 0).sum()))


def check_window(W, lim, tick_q, tick):
    """rule 48: (step_q, R_q); ValueError where the call answers WA_ERR_ARG"""
    if not isinstance(W, (int, np.integer)) or W < 1 or W > MAX_W:
        raise ValueError("window")
    step = np.floor((np.float64(lim["v_max"]) * np.float64(tick)) * QF)
    if not step < float(CAP):
        raise ValueError("reach")
    step_q = int(step) + 1
    R_q = (int(W) - 1) * step_q
    if R_q >= CAP or (int(W) - 1) * tick_q >= CAP:
        raise ValueError("reach or window time reaches 2^61")
    return step_q, R_q


def retime_jerk(xyz, lim, dwell=None, window=1, v_limit=None, grid=None, tick=0.01, seg_tag=None, want_tags=None, want_ticks=True,
                lower=True):
    """wa_traj_retime_jerk: dict(time_q, w_q, bound, ticks float32[n_ticks, 3], s_q, tag, summary, stops, jerk, and what the tests look
    at: U, C13, kind13, Cl, GL, L, seg, rest); ValueError where the call answers WA_ERR_ARG.  Above 2^31 output ticks ticks, s_q and tag
    are None and the jerk summary's tick fields 0 (WA_ERR_CAPACITY)."""
    base = R.retime(xyz, lim, v_limit, grid, tick, False)   # (the arguments of retime rule 7)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    tick_q = base["tick_q"]
    W = window
    _, R_q = check_window(W, lim, tick_q, tick)
    W = int(W)
    if not lower:
        R_q = 0
    want_tags = seg_tag is not None if want_tags is None else want_tags
    if want_tags and seg_tag is None:
        raise ValueError("tag_out without seg_tag")
    if seg_tag is not None:
        seg_tag = np.asarray(seg_tag, np.uint8).reshape(-1)
        if len(seg_tag) != n - 1:
            raise ValueError("seg_tag")
    dq = np.full(n - 1, -1, np.int64) if dwell is None else S.dwell_quanta(dwell, n)
    stop = dq >= 0
    ext = (W - 1) * tick_q
    if stop.any() and int(dq.max()) + ext >= CAP:
        raise ValueError("an extended dwell reaches 2^61")
    ds, L, A, D = base["ds"], base["L"], base["A"], base["D"]
    if (stop & (L > 0)).any():
        raise ValueError("a stop on a segment that has a length")
    length_q = int(L.sum())
    if W * length_q >= (1 << 62):
        raise ValueError("W * length reaches 2^62")
    GL = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    # rules 49 - 51: lowered caps, extended dwells, the profile
    C13, kind13 = caps13(xyz, lim, v_limit, grid)
    Cl, kindl = lowered_caps(C13, kind13, GL, R_q)
    low = Cl < C13
    at_stop = np.zeros(n, bool)
    at_stop[:-1] |= stop
    at_stop[1:] |= stop
    stop_sample = at_stop.copy()
    at_stop[0] = at_stop[-1] = True   # (kind 0: the end points and both samples of every stop)
    C = np.where(at_stop, 0, Cl).astype(np.int64)
    kind = np.where(at_stop, R.KIND_END, kindl).astype(np.uint8)
    F, B = R.passes(C, A, D)
    bound = (R.bound_bits(C, B, A, D, kind) | np.where(low, LOWERED, 0).astype(np.uint8)).astype(np.uint8)
    dt, T, tri, t_up = R.times(ds, L, B, lim["acc"], lim["dec"])
    T = np.where(stop, dq + ext, T).astype(np.int64)
    if S._big_sum(T) >= CAP:
        raise ValueError("duration reaches 2^61")
    time_q = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    time = int(time_q[-1])
    n_u = R.tick_count(time, tick_q)
    summary = dict(n=n, n_ticks=n_u, length_q=length_q, time_q=time, n_bound=[int((kind == k).sum()) for k in range(4)],
                   n_on_cap=int((bound & 1).astype(bool).sum()), n_on_ramp=int((bound & 6).astype(bool).sum()),
                   n_triangle=int(tri.sum()), n_outside=base["summary"]["n_outside"], peak_w_q=int(B.max()))
    stops = dict(n_stops=int(stop.sum()), n_stop_samples=int(stop_sample.sum()), dwell_q=int(dq[stop].sum()))   # (the caller's own dwells)
    out = dict(time_q=time_q, w_q=B, bound=bound, summary=summary, stops=stops, C13=C13, kind13=kind13, Cl=Cl, C=C, kind=kind, GL=GL, L=L,
               dq=dq, tick_q=tick_q, ticks=None, s_q=None, tag=None, U=None, seg=None, rest=None)
    n_ticks = n_u + W - 1
    if n_ticks > R.MAX_TICKS:
        out["jerk"] = dict(window=W, reach_q=R_q, n_lowered=int(low.sum()), n_in=n_u, n_ticks=n_ticks, max_d1=0, max_d2=0, max_d3=0,
                           in_max_d2=0, n_rest_ticks=0, n_short_rests=0, n_back=0)
        return out
    # rules 52 - 54: unfiltered arc lengths, the filter, where a tick lies
    U = arcs(xyz, L, GL, time_q, B, lim["acc"], lim["dec"], tick_q)
    S_q = window_means(U, W, length_q)
    seg, rest, at_end = locate(S_q, GL, L, stop)
    out["jerk"] = summary_of(S_q, U, W, length_q, R_q, low.sum(), rest, seg, GL, stop, dq, tick_q)
    out.update(U=U, s_q=S_q, seg=seg, rest=rest)
    if want_ticks:
        out["ticks"] = positions(xyz, S_q, GL, L, seg, rest, at_end)
    if want_tags:
        out["tag"] = seg_tag[seg]
    return out


def retime_jerk_scalar(xyz, lim, dwell=None, window=1, v_limit=None, grid=None, tick=0.01, seg_tag=None):
    """rules 52 - 54 once more, one tick after the other with Python integers and an explicit window sum, on the profile of the array
    form: (s_q list, segments list, rest flags list, positions float32[n_ticks, 3], tags list or None)"""
    r = retime_jerk(xyz, lim, dwell, window, v_limit, grid, tick, seg_tag, want_ticks=False)
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    n, W = len(p32), int(window)
    GL, L = [int(x) for x in r["GL"]], [int(x) for x in r["L"]]
    stop = [int(x) >= 0 for x in r["dq"]]
    length_q = GL[-1]
    _, ti, lam, _ = K.tick_params(p32, r["time_q"], r["w_q"], lim["acc"], lim["dec"], r["tick_q"])
    U = []
    for k in range(len(ti)):
        i = int(ti[k])
        tau = min(k * r["tick_q"], int(r["time_q"][-1]))
        if tau >= int(r["time_q"][i + 1]):
            x = L[i]
        elif L[i] == 0:
            x = 0
        else:
            x = int(np.rint(np.float64(lam[k]) * np.float64(L[i])))
        U.append(GL[i] + x)
    n_u = len(U)
    u_at = lambda k: 0 if k < 0 else (length_q if k >= n_u else U[k])
    s_q, segs, rests, tags = [], [], [], []
    pos = np.empty((n_u + W - 1, 3), np.float32)
    stops = [i for i in range(n - 1) if stop[i]]
    for k in range(n_u + W - 1):
        s = sum(u_at(j) for j in range(k - W + 1, k + 1)) // W
        s_q.append(s)
        hit = [i for i in stops if GL[i] == s]
        if hit:
            i = hit[0]
            pos[k] = p32[i]
        else:
            i = min(bisect.bisect_right(GL, s), n - 1) - 1   # (the last segment m with GL[m] <= s; GL never falls)
            if s >= GL[i + 1]:
                pos[k] = p32[i + 1]
            elif L[i] == 0:
                pos[k] = p32[i]
            else:
                lm = np.float64(s - GL[i]) / np.float64(L[i])
                a, b = p32[i].astype(np.float64), p32[i + 1].astype(np.float64)
                pos[k] = (a + (b - a) * lm).astype(np.float32)
        segs.append(i)
        rests.append(bool(hit))
        if seg_tag is not None:
            tags.append(int(seg_tag[i]))
    return s_q, segs, rests, pos, tags if seg_tag is not None else None


# ------------------------------------------------------------------ what the tests hold the definition against
def speed_excess(r, tick):
    """the largest S_(k+1) - S_k - tick * sqrt(max(C13[i0 .. i1]) / Q) * Q over the filtered ticks, in quanta: i0 the segment rule 54 (b)
    gives for S_k, i1 the first sample with GL >= S_(k+1), at least i0 + 1"""
    S_q, GL, C13 = r["s_q"], r["GL"], r["C13"]
    n = len(GL)
    a, b = S_q[:-1], S_q[1:]
    i0 = np.minimum(np.searchsorted(GL, a, side="right") - 1, n - 2)
    i1 = np.maximum(np.searchsorted(GL, b, side="left"), i0 + 1)
    key = (~C13.astype(np.uint64))   # (a range MAXIMUM by the minimum of the complements)
    cmax = (~range_min(key, i0, i1)).astype(np.int64)
    allow = np.float64(tick) * np.sqrt(cmax.astype(np.float64) / QF) * QF
    return float(((b - a).astype(np.float64) - allow).max())


def rest_ticks_per_stop(r):
    """rest ticks taken by every stop segment (the lowest-numbered stop of a group takes the group's)"""
    return np.bincount(r["seg"][r["rest"]], minlength=len(r["GL"]))[np.flatnonzero(r["dq"] >= 0)]
