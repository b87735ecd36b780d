"""numpy restatement of the tool poses at controller ticks (include/weldacs.h rules 24 - 26: wa_traj_axes_smooth, wa_traj_axes_limits,
wa_traj_tick_axes), written from the header's definition and independent of the kernels: int64 and individually rounded float64
operations.  L, the segment times and rule 6 come from retime_ref, the bead rule and the voxel lookup from torch_ref (which uses
clearance_ref's distance field); grid = (free, d2, dims, axes) as retime_ref.make_grid returns it.  No GPU, no product code.

Axes are quantised integers q (int64 here, n x 3, |q_c| <= 16384, no all-zero triple): torch_ref.quantise_all makes them from floats."""
import numpy as np

import clearance_ref as CR  # noqa: F401  (the distance field behind retime_ref.make_grid / torch_ref.make_grid)
import retime_ref as R
import torch_ref as T

Q = R.Q
QF = R.QF
CAP = R.CAP_INF
MAX_LEVEL = 8
MAX_LEG = 1 << 22
SMOOTH_FIELDS = ("n", "n_outside", "n_level", "n_blocked", "first_blocked", "n_zero_sum", "max_turn_in", "max_turn_out")
LIMITS_FIELDS = ("n", "n_turning", "n_jump", "n_floored", "n_limited", "min_limit")
TICK_FIELDS = ("n_ticks", "n_outside", "n_blocked", "first_blocked", "n_near", "max_tick_turn")


def check_axes(q, n):
    q = np.asarray(q, np.int64).reshape(-1, 3)
    if len(q) != n or (np.abs(q) > 16384).any() or (q == 0).all(1).any():
        raise ValueError("axes")
    return q


def lengths(xyz):
    """(ds float64[n-1], L int64[n-1], GL int64[n]) -- retime rule 1; ValueError where the total reaches 2^61"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("not finite")
    ds = R.seg_lengths(xyz)
    L = R._quanta(ds)
    if sum(int(x) for x in L[L >= (1 << 40)]) + int(L[L < (1 << 40)].sum()) >= CAP:
        raise ValueError("sum reaches 2^61")
    return ds, L, np.concatenate([[0], np.cumsum(L)]).astype(np.int64)


def quantise_rows(v):
    """rule 1 on float64 rows that are not all zero"""
    v = np.asarray(v, np.float64)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return np.rint((v / ln[:, None]) * 16384.0).astype(np.int64)


def windows(GL, off, idx, w):
    """(first, last) sample of the window of half-width w (quanta) around each sample of idx, cut at the legs of off"""
    lo, hi = np.empty(len(idx), np.int64), np.empty(len(idx), np.int64)
    leg = np.searchsorted(off, idx, side="right") - 1          # the largest l with off[l] <= i: empty legs are passed over
    for l in np.unique(leg):
        m = leg == l
        s, e = int(off[l]), int(off[l + 1])
        g = GL[s:e]
        gi = GL[idx[m]]
        lo[m] = s + np.searchsorted(g, gi - w, side="left")
        hi[m] = s + np.searchsorted(g, gi + w, side="right") - 1
    return lo, hi


def window_sums(q, lo, hi):
    P = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(q, axis=0)])
    return P[hi + 1] - P[lo]


def candidates(q, GL, off, idx, w):
    """(candidate int64[len(idx), 3], zero-sum mask) at window half-width w"""
    lo, hi = windows(GL, off, idx, w)
    S = window_sums(q, lo, hi)
    zero = (S == 0).all(1)
    c = q[idx].copy()
    if (~zero).any():
        c[~zero] = quantise_rows(S[~zero].astype(np.float64))
    return c, zero


def blocked_at(grid, vox, q, tool, near_add=-1):
    """rule 2 for one axis per voxel: (blocked bool, near count)"""
    dist16, r2 = tool
    b, m = T.beads(grid, vox, T.offsets(q, dist16), r2, near_add)
    return b.any(-1), m.sum(-1)


def smooth(xyz, q, h, max_level, grid=None, tool=None, off=None):
    """wa_traj_axes_smooth: dict(q, level, blocked, summary); ValueError where the call answers WA_ERR_ARG, OverflowError for a long leg"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    if n < 1 or (grid is None) != (tool is None) or not 0 <= max_level <= MAX_LEVEL or not np.isfinite(h) or h < 0:
        raise ValueError("arguments")
    hq = np.rint(np.float64(h) * QF)
    if not hq <= float(CAP):
        raise ValueError("h")
    h_q = int(hq)
    off = np.asarray([0, n] if off is None else off, np.int64)
    if len(off) < 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError("off")
    q = check_axes(q, n)
    if (np.diff(off) > MAX_LEG).any():
        raise OverflowError("leg")
    _, _, GL = lengths(xyz)
    n_outside = 0
    vox = None
    if grid is not None:
        vox, outside = T.sample_voxels(grid, xyz)
        n_outside = int(outside.sum())
    q_out = q.copy()
    level = np.zeros(n, np.uint8)
    blocked = np.zeros(n, np.uint8)
    zero_chosen = np.zeros(n, bool)
    todo = np.arange(n)
    for lev in range(max_level + 1):
        if lev < max_level:
            c, zero = candidates(q, GL, off, todo, h_q >> lev)
        else:
            c, zero = q[todo].copy(), np.zeros(len(todo), bool)
        blk = blocked_at(grid, vox[todo], c, tool)[0] if grid is not None else np.zeros(len(todo), bool)
        done = ~blk if lev < max_level else np.ones(len(todo), bool)
        d = todo[done]
        q_out[d], level[d], blocked[d], zero_chosen[d] = c[done], lev, blk[done], zero[done]
        todo = todo[~done]
        if not len(todo):
            break
    inner = np.ones(max(n - 1, 0), bool)
    inner[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < n)] - 1] = False     # pairs (i, i + 1) that straddle a leg boundary
    t_in = T.turn(q[:-1], q[1:])[inner]
    t_out = T.turn(q_out[:-1], q_out[1:])[inner]
    summary = dict(n=n, n_outside=n_outside, n_level=[int((level == l).sum()) for l in range(MAX_LEVEL + 1)], n_blocked=int(blocked.sum()),
                   first_blocked=int(np.flatnonzero(blocked)[0]) if blocked.any() else -1, n_zero_sum=int(zero_chosen.sum()),
                   max_turn_in=int(t_in.max()) if len(t_in) else 0, max_turn_out=int(t_out.max()) if len(t_out) else 0)
    return dict(q=q_out, level=level, blocked=blocked, summary=summary)


def floats_below(lim):
    """the largest float32 <= lim (lim >= 0)"""
    with np.errstate(over="ignore"):
        f = np.asarray(lim, np.float64).astype(np.float32)
    up = f.astype(np.float64) > lim
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def limits(xyz, q, omega, v_cap, v_floor, v_limit_in=None):
    """wa_traj_axes_limits: dict(v_limit float32[n], summary, psi, D, L, floored)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    fin = lambda x: np.isfinite(x) and x > 0
    if n < 1 or not (fin(omega) and fin(v_cap) and fin(v_floor)) or v_floor > v_cap:
        raise ValueError("arguments")
    floor_f = np.float32(v_floor)
    if np.float64(floor_f) < v_floor:
        floor_f = np.nextafter(floor_f, np.float32(np.inf))
    if not np.isfinite(floor_f):
        raise ValueError("v_floor")
    q = check_axes(q, n)
    if v_limit_in is not None:
        v_limit_in = np.asarray(v_limit_in, np.float32)
        if len(v_limit_in) != n or not (np.isfinite(v_limit_in) & (v_limit_in > 0)).all():
            raise ValueError("v_limit_in")
    if not np.isfinite(xyz).all():
        raise ValueError("not finite")
    ds = R.seg_lengths(xyz)
    L = R._quanta(ds)
    d = q[:-1] - q[1:]
    D = (d * d).sum(1)
    psi = np.sqrt(D.astype(np.float64)) / 16384.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        m = (ds * np.float64(omega)) / psi
    m = np.where((D > 0) & (L > 0), m, np.inf)
    lim = np.full(n, np.float64(v_cap))
    lim[1:] = np.minimum(lim[1:], m)
    lim[:-1] = np.minimum(lim[:-1], m)
    if v_limit_in is not None:
        lim = np.minimum(lim, v_limit_in.astype(np.float64))
    f = floats_below(lim)
    floored = f.astype(np.float64) < v_floor
    f = np.where(floored, floor_f, f).astype(np.float32)
    summary = dict(n=n, n_turning=int((D > 0).sum()), n_jump=int(((D > 0) & (L == 0)).sum()), n_floored=int(floored.sum()),
                   n_limited=int((f.astype(np.float64) < v_cap).sum()), min_limit=float(f.min()))
    return dict(v_limit=f, summary=summary, psi=psi, D=D, L=L, floored=floored)


def tick_params(xyz, time_q, w_q, acc, dec, tick_q):
    """rule 6 per tick: (taus, segment i, lambda with the exact cases as 1 and 0, positions float32)"""
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    n = len(p)
    time_q, B = np.asarray(time_q, np.int64), np.asarray(w_q, np.int64)
    ds = R.seg_lengths(p32)
    L = R._quanta(ds)
    dt, _, tri, t_up = R.times(ds, L, B, acc, dec)
    total = int(time_q[-1])
    taus = np.arange(total // tick_q + 1, dtype=np.int64) * np.int64(tick_q)
    if total % tick_q:
        taus = np.concatenate([taus, [total]])
    i = np.searchsorted(time_q[:n - 1], taus, side="right") - 1
    e = (taus - time_q[i]).astype(np.float64) / QF
    acc, dec = np.float64(acc), np.float64(dec)
    v = np.sqrt(B.astype(np.float64) / QF)
    dsi = ds[i]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = ((B[i + 1] - B[i]).astype(np.float64) / QF) / (np.float64(2.0) * dsi)
        s_c = (v[i] * e) + ((np.float64(0.5) * a) * e) * e
        r = dt[i] - e
        s_b = np.where(e <= t_up[i], ((np.float64(0.5) * acc) * e) * e, dsi - ((np.float64(0.5) * dec) * r) * r)
        lam = np.where(tri[i], s_b, s_c) / dsi
    lam = np.where(lam < 0.0, 0.0, np.where(lam > 1.0, 1.0, lam))
    at_end = taus >= time_q[i + 1]
    still = (L[i] == 0) & ~at_end
    lam = np.where(at_end, 1.0, np.where(still, 0.0, lam))
    pos = (p[i] + (p[i + 1] - p[i]) * lam[:, None]).astype(np.float32)
    pos[still] = p32[i[still]]
    pos[at_end] = p32[i[at_end] + 1]
    return taus, i, lam, pos


def tick_axes(xyz, q, time_q, w_q, acc, dec, tick, grid=None, tool=None, near_add=-1):
    """wa_traj_tick_axes: dict(axes float32[n_ticks, 3], qt, blocked uint8[n_ticks], pos, summary); OverflowError above 2^31 ticks"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    fin = lambda x: np.isfinite(x) and x > 0
    if n < 2 or (grid is None) != (tool is None) or not (fin(acc) and fin(dec)) or not np.isfinite(tick):
        raise ValueError("arguments")
    tq = np.rint(np.float64(tick) * QF)
    if not (tq >= 1 and tq <= float(CAP)):
        raise ValueError("tick")
    tick_q = int(tq)
    time_q, w_q = np.asarray(time_q, np.int64), np.asarray(w_q, np.int64)
    if len(time_q) != n or len(w_q) != n or time_q[0] != 0 or (np.diff(time_q) < 0).any() or (time_q >= CAP).any() or (w_q < 0).any() \
            or (w_q > CAP).any():
        raise ValueError("times")
    if tool is not None and near_add > (1 << 30):
        raise ValueError("near_add")
    q = check_axes(q, n)
    if not np.isfinite(xyz).all():
        raise ValueError("not finite")
    if R.tick_count(int(time_q[-1]), tick_q) > R.MAX_TICKS:
        raise OverflowError("ticks")
    _, i, lam, pos = tick_params(xyz, time_q, w_q, acc, dec, tick_q)
    qa, qb = q[i].astype(np.float64), q[i + 1].astype(np.float64)
    v = qa + (qb - qa) * lam[:, None]
    zero = (v == 0).all(1)
    qt = q[i].copy()
    qt[~zero] = quantise_rows(v[~zero])
    axes = (qt.astype(np.float64) / 16384.0).astype(np.float32)
    k = len(i)
    blocked, near, n_outside = np.zeros(k, bool), np.zeros(k, np.int64), 0
    if grid is not None:
        vox, outside = T.sample_voxels(grid, pos)
        n_outside = int(outside.sum())
        blocked, near = blocked_at(grid, vox, qt, tool, near_add)
    turn = T.turn(qt[:-1], qt[1:])
    summary = dict(n_ticks=k, n_outside=n_outside, n_blocked=int(blocked.sum()), first_blocked=int(np.flatnonzero(blocked)[0]) if blocked.any() else -1,
                   n_near=int((~blocked & (near > 0)).sum()), max_tick_turn=int(turn.max()) if len(turn) else 0)
    return dict(axes=axes, qt=qt, blocked=blocked.astype(np.uint8), pos=pos, summary=summary, i=i, lam=lam)


# ------------------------------------------------------------------ scenes for the tests
def stepped_axes(n, every=7, K=32, half_angle=1.2, axis=(0.0, 0.0, 1.0)):
    """a new direction of torch_ref.fib_dirs(K) every `every` samples: what wa_traj_tool_axes hands on, piecewise constant"""
    d = T.quantise_all(T.fib_dirs(K, half_angle, axis))
    return d[(np.arange(n) // every) % K]


def slab_turn_scene(per_leg=60):
    """retime_ref.slab_scene's grid (metal: x in 10..13, y in 0..5, all z) and a pass along y = 8, z = 4 from x = 1 to x = 22 whose axis
    turns by 90 degrees over the middle of the slab (x = 11.5): (-1, -1, 0) / sqrt 2 before, (+1, -1, 0) / sqrt 2 after.  Either axis
    leans away from the slab's middle and its rod passes the slab's corner; their average (0, -1, 0) points straight into the metal.
    So a wide window around the change is blocked, a narrow one is not: the level climbs.  Returns (grid, xyz, q, tool)."""
    grid, _ = R.slab_scene()
    xyz = R.densify([[1, 8, 4], [22, 8, 4]], per_leg)
    q = np.where((xyz[:, 0] < 11.5)[:, None], np.array([-11585, -11585, 0]), np.array([11585, -11585, 0])).astype(np.int64)
    return grid, xyz, q, T.rod(8, 16 * 6, 0)
