"""numpy restatement of the torch axes at jerk-limited ticks (include/weldacs.h rules 56 - 60: wa_traj_retime_jerk_axes), assembled by
import from jerk_ref (rules 48 - 55: the profile, S_k, the segment or stop of every filtered tick, its position and tag) and ticks_ref
(rule 1's quantisation, rule 26's expression through quantise_rows, the bead rule and the voxel lookup).  What is stated here is the
axis of a moving tick (rule 57), the turn in place over the rest ticks of a stop (rule 58) and the summary (rule 60).  No GPU, no
product code.

`grid` serves both the caps of the profile (retime rule 2, kind 3) and the bead check, as the call's one grid does."""
import numpy as np

import jerk_ref as J
import ticks_ref as K

T = K.T
AXES_FIELDS = ("n_ticks", "n_outside", "n_blocked", "first_blocked", "n_near", "max_tick_turn", "n_rest_ticks", "n_turning_rests",
               "min_turn_ticks", "max_rest_turn")
MAX_BEADS = 64


def check_tool(tool, near_add):
    """rule 9: ValueError where the call answers WA_ERR_ARG"""
    dist16, r2 = (np.asarray(x, np.int64).reshape(-1) for x in tool)
    if len(dist16) != len(r2) or not 1 <= len(r2) <= MAX_BEADS or near_add > (1 << 30):
        raise ValueError("tool")
    if (dist16 < 0).any() or (dist16 > 65536).any() or (r2 < 0).any() or (r2 > (1 << 30)).any():
        raise ValueError("tool")


def interpolate(qa, qb, lam):
    """rule 26's expression between the rows of qa and qb, quantised by rule 1; qa where it is all zero"""
    v = qa.astype(np.float64) + (qb.astype(np.float64) - qa.astype(np.float64)) * np.asarray(lam, np.float64)[:, None]
    zero = (v == 0).all(1)
    qt = qa.copy()
    if (~zero).any():
        qt[~zero] = K.quantise_rows(v[~zero])
    return qt, zero


def runs(GL, f):
    """rule 58: (a, e) -- the lowest and the highest sample index with GL = GL_f"""
    return np.searchsorted(GL, GL[f], side="left"), np.searchsorted(GL, GL[f], side="right") - 1


def rest_counts(seg, rest, n):
    """rule 58 by counting: (first int64[n], R int64[n]) per stop segment; first = n_ticks where no tick rests"""
    k = np.flatnonzero(rest)
    first = np.full(n, len(seg), np.int64)
    np.minimum.at(first, seg[k], k)
    return first, np.bincount(seg[k], minlength=n).astype(np.int64)


def axes_of(r, q):
    """rules 57 and 58 on jerk_ref's dictionary: (qt int64[n_ticks, 3], lambda float64, zero mask, first, R)"""
    S_q, GL, L, seg, rest = r["s_q"], r["GL"], r["L"], r["seg"], r["rest"]
    n = len(GL)
    k = np.arange(len(S_q), dtype=np.int64)
    first, R = rest_counts(seg, rest, n)
    i = seg
    at_end = ~rest & (S_q >= GL[i + 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (S_q - GL[i]).astype(np.float64) / L[i].astype(np.float64)
        lam = np.where(at_end, 1.0, np.where(L[i] == 0, 0.0, lam))
        lam_rest = (k - first[i]).astype(np.float64) / R[i].astype(np.float64)
    lam = np.where(rest, np.clip(lam_rest, 0.0, 1.0), lam)
    a, e = runs(GL, i)
    ia, ib = np.where(rest, a, i), np.where(rest, e, i + 1)
    qt, zero = interpolate(q[ia], q[ib], lam)
    return qt, lam, zero, first, R


def groups(r, q, R):
    """rule 60: (heads of the stop groups, their q_a != q_e mask)"""
    GL, stop = r["GL"], r["dq"] >= 0
    heads = np.asarray(sorted({int(np.flatnonzero(stop & (GL[:-1] == g))[0]) for g in set(GL[:-1][stop].tolist())}), np.int64)
    a, e = runs(GL, heads)
    return heads, (q[a] != q[e]).any(1)


def retime_jerk_axes(xyz, q, lim, dwell=None, window=1, v_limit=None, grid=None, tool=None, near_add=-1, tick=0.01, seg_tag=None):
    """wa_traj_retime_jerk_axes: jerk_ref.retime_jerk's dictionary plus axes float32[n_ticks, 3], qt, blocked uint8[n_ticks], axes_summary
    and what the tests look at (lam, zero, first, R); ValueError where the call answers WA_ERR_ARG.  Above 2^31 ticks axes, qt and
    blocked are None and the axes summary all zero."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    if q is None or (grid is None) != (tool is None) or n < 2:
        raise ValueError("arguments")
    if tool is not None:
        check_tool(tool, near_add)
    q = K.check_axes(q, n)
    r = J.retime_jerk(xyz, lim, dwell, window, v_limit, grid, tick, seg_tag)
    if r["s_q"] is None:
        return dict(r, axes=None, qt=None, blocked=None, axes_summary=dict.fromkeys(AXES_FIELDS, 0))
    qt, lam, zero, first, R = axes_of(r, q)
    rest = r["rest"]
    m = len(qt)
    blocked, near, n_outside = np.zeros(m, bool), np.zeros(m, np.int64), 0
    if grid is not None:
        vox, outside = T.sample_voxels(grid, r["ticks"])
        n_outside = int(outside.sum())
        blocked, near = K.blocked_at(grid, vox, qt, tool, near_add)
    turn = np.concatenate([[0], T.turn(qt[:-1], qt[1:])]).astype(np.int64)
    heads, turning = groups(r, q, R)
    summary = dict(n_ticks=m, n_outside=n_outside, n_blocked=int(blocked.sum()),
                   first_blocked=int(np.flatnonzero(blocked)[0]) if blocked.any() else -1, n_near=int((~blocked & (near > 0)).sum()),
                   max_tick_turn=int(turn.max()), n_rest_ticks=int(rest.sum()), n_turning_rests=int(turning.sum()),
                   min_turn_ticks=int(R[heads[turning]].min()) if turning.any() else 0, max_rest_turn=int(turn[rest].max()) if rest.any() else 0)
    assert summary["n_rest_ticks"] == r["jerk"]["n_rest_ticks"]
    return dict(r, axes=(qt.astype(np.float64) / 16384.0).astype(np.float32), qt=qt, blocked=blocked.astype(np.uint8), axes_summary=summary,
                lam=lam, zero=zero, first=first, R=R, turn=turn)


def retime_jerk_axes_scalar(xyz, q, lim, dwell=None, window=1, v_limit=None, grid=None, tick=0.01):
    """rules 57 and 58 once more, one tick after the other with Python integers, on jerk_ref's own per-tick loop: the axes as a list
    of integer triples"""
    s_q, segs, rests, _, _ = J.retime_jerk_scalar(xyz, lim, dwell, window, v_limit, grid, tick)
    r = J.retime_jerk(xyz, lim, dwell, window, v_limit, grid, tick, want_ticks=False)
    GL, L = [int(x) for x in r["GL"]], [int(x) for x in r["L"]]
    n = len(GL)
    q = [[int(c) for c in row] for row in K.check_axes(q, n)]

    def mix(qa, qb, lam):
        v = [np.float64(qa[c]) + (np.float64(qb[c]) - np.float64(qa[c])) * lam for c in range(3)]
        if all(x == 0 for x in v):
            return list(qa)
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [int(np.rint((x / ln) * np.float64(16384.0))) for x in v]

    out, ticks_of = [], {}
    for k, (s, i, rest) in enumerate(zip(s_q, segs, rests)):
        if rest:
            mine = ticks_of.setdefault(i, [j for j in range(len(s_q)) if rests[j] and segs[j] == i])
            same = [j for j in range(n) if GL[j] == GL[i]]
            lam = np.float64(k - mine[0]) / np.float64(len(mine))
            out.append(mix(q[same[0]], q[same[-1]], min(max(lam, np.float64(0.0)), np.float64(1.0))))
        elif s >= GL[i + 1]:
            out.append(mix(q[i], q[i + 1], np.float64(1.0)))
        elif L[i] == 0:
            out.append(mix(q[i], q[i + 1], np.float64(0.0)))
        else:
            out.append(mix(q[i], q[i + 1], np.float64(s - GL[i]) / np.float64(L[i])))
    return out


# ------------------------------------------------------------------ scenes for the tests
def wall_grid(m, at=None, upto=None):
    """an m^3 grid (unit axes) whose only metal is one wall: x = at (m // 2), y < upto (0.6 m), every z"""
    free = np.ones((m, m, m), np.uint8)   # [z, y, x]
    free[:, :int(0.6 * m) if upto is None else upto, m // 2 if at is None else at] = 0
    return T.make_grid(free, (m, m, m))


def polyline(pieces):
    """pieces: (points float[k, 3], joint) -- a piece begins where the one before it ends (a piece may be that one point alone); joint
    lists the dwells of the segments without length put in front of it, < 0 for one that is no stop ([] joins the pieces as they
    are).  Returns (xyz float32, dwell float64[n-1])."""
    parts, dwell = [], []
    for k, (pts, joint) in enumerate(pieces):
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        if k:
            assert np.array_equal(pts[0], parts[-1][-1])
            parts.append(np.repeat(pts[:1], len(joint), 0))
            dwell += [float(d) for d in joint]
            pts = pts[1:]
            dwell += [-1.0] * len(pts)
        else:
            dwell += [-1.0] * (len(pts) - 1)
        parts.append(pts)
    return np.concatenate(parts).astype(np.float32), np.asarray(dwell, np.float64)


def fixed_axis(v):
    """a quantised axis near v that rule 1 maps to itself (quantising a quantised triple again can move a component by 1: iterate)"""
    q = T.quantise_all([v])
    for _ in range(8):
        q2 = K.quantise_rows(q.astype(np.float64))
        if np.array_equal(q, q2):
            return q[0]
        q = q2
    raise AssertionError("no fixed point near %r" % (v,))


def random_case(seed):
    """a seeded case of 2 .. 40 samples in a 16^3 .. 24^3 grid with one wall: legs of 1 - 5 samples, at the joints (and now and then at
    the very start) runs of 1 - 3 repeated samples whose segments are stops of 0, 0.05 or 0.2 s or no stops at all (every fifth case comes
    without a dwell array); random axes, now and then held over a few samples or reversed; a tool of 1 - 3 beads.  Returns dict(grid, xyz, q, dwell, lim, tick, tool, near_add,
    tag)."""
    import retime_ref as R
    rs = np.random.RandomState(1000 + seed)
    m = int(rs.randint(16, 25))
    pts, dwell = [rs.uniform(1.0, m - 2.0, 3)], []

    def run():
        for _ in range(int(rs.choice([0, 0, 1, 2, 3]))):
            pts.append(pts[-1])
            dwell.append(float(rs.choice([-1.0, 0.0, 0.05, 0.2])))

    if seed % 4 == 0:
        run()
    for _ in range(int(rs.randint(1, 6))):
        b, per = rs.uniform(1.0, m - 2.0, 3), int(rs.randint(1, 6))
        a = pts[-1]
        for j in range(1, per + 1):
            pts.append(a + (b - a) * (j / per))
            dwell.append(-1.0)
        run()
        if len(pts) >= 34:
            break
    xyz = np.asarray(pts, np.float32)   # (a repeated sample is the same float64 triple: the same fp32 point)
    n = len(xyz)
    v = rs.normal(size=(n, 3))
    for i in range(1, n):
        u = rs.uniform()
        if u < 0.3:
            v[i] = v[i - 1]
        elif u < 0.4:
            v[i] = -v[i - 1]
    q = T.quantise_all(v)
    for i in range(1, n):   # (a reversed axis is the exact negative)
        if np.array_equal(v[i], -v[i - 1]):
            q[i] = -q[i - 1]
    lim = R.limits(v_max=rs.uniform(4.0, 10.0), acc=rs.uniform(8.0, 20.0), dec=rs.uniform(8.0, 20.0), a_lat=rs.uniform(2.0, 20.0),
                   v_near=rs.uniform(1.0, 3.0), near_d2=int(rs.randint(1, 6)))
    tool = T.rod(int(rs.randint(1, 4)), 16 * int(rs.randint(2, 7)), int(rs.randint(0, 3)))
    return dict(grid=wall_grid(m), xyz=xyz, q=q, dwell=np.asarray(dwell, np.float64) if seed % 5 != 3 else None,
                lim=lim, tick=float(rs.choice([0.01, 0.02])), tool=tool, near_add=int(rs.choice([-1, 0, 3])),
                tag=(np.arange(n - 1) % 250 + 1).astype(np.uint8))
