"""numpy restatement of wa_traj_retime (include/weldacs.h): rules 1 - 6 of the header's definition with explicit float32 / float64 / int64
operations, vectorised through the closed forms of rule 3 (a prefix minimum and a suffix minimum), plus the sequential recurrences of
rule 3 as a second implementation, plus scene builders.  No GPU, no product code.

Q = 2^30.  Samples p_0 .. p_{n-1} (fp32, n >= 2), segment i joins p_i and p_{i+1}.
1. Lengths.  ds_i = sqrt((dx*dx + dy*dy) + dz*dz) in float64 on the fp32 coordinates.  L_i = rint(ds_i * Q), A_i = rint(((2 * acc) * ds_i) * Q),
   D_i likewise with dec; where L_i > 0 both are raised to at least 1, where L_i = 0 both are 0.  GA, GD = exclusive prefix sums.
2. Caps (squared speeds, float64), the minimum of: kind 0 the end points (0); kind 1 min(v_max, v_limit[i])^2; kind 2 (interior samples)
   a_lat over the Menger curvature (2 c) / den; kind 3 v_near^2 where the sample's voxel has d2 <= near_d2.  kind = the lowest-numbered kind
   attaining the minimum.  C_i = floor(cap * Q), 2^61 where that is infinite or >= 2^61.
3. F_0 = C_0, F_i = min(C_i, F_{i-1} + A_{i-1}); B_{n-1} = F_{n-1}, B_i = min(F_i, B_{i+1} + D_i).
4. bound: bit 0 B_i = C_i; bit 1 i > 0 and B_i - B_{i-1} = A_{i-1}; bit 2 i < n-1 and B_i - B_{i+1} = D_i; bits 4-5 the kind.
5. Times.  v_i = sqrt((double)B_i / Q); (a) L_i = 0: dt = 0; (b) L_i > 0 and v_i + v_{i+1} = 0: the rest-to-rest triangle; (c) else
   dt = (2 ds) / (v_i + v_{i+1}).  T_i = rint(dt * Q); time_q = the exclusive prefix sum.
6. Ticks at k * tick_q and at the duration: the position on the segment by the constant-acceleration law of the segment."""
import numpy as np

Q = 1 << 30
QF = np.float64(Q)
CAP_INF = 1 << 61
MAX_TICKS = 1 << 31
KIND_END, KIND_VMAX, KIND_CURV, KIND_NEAR = 0, 1, 2, 3


def limits(v_max=1.0, acc=1.0, dec=1.0, a_lat=np.inf, v_near=1.0, near_d2=-1):
    return dict(v_max=float(v_max), acc=float(acc), dec=float(dec), a_lat=float(a_lat), v_near=float(v_near), near_d2=int(near_d2))


def _norm(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def seg_lengths(xyz):
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    return _norm(p[1:] - p[:-1])


def _quanta(x):
    """rint(x * Q) as int64, 2^61 where that is >= 2^61"""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(np.asarray(x, np.float64) * QF)
    big = ~(q < float(CAP_INF))
    return np.where(big, CAP_INF, np.where(big, 0.0, q).astype(np.int64)).astype(np.int64)


def segments(xyz, acc, dec):
    """(ds float64, L, A, D int64) per segment -- rule 1"""
    ds = seg_lengths(xyz)
    L = _quanta(ds)
    A = _quanta((np.float64(2.0) * np.float64(acc)) * ds)
    D = _quanta((np.float64(2.0) * np.float64(dec)) * ds)
    pos = L > 0
    A = np.where(pos, np.maximum(A, 1), 0).astype(np.int64)
    D = np.where(pos, np.maximum(D, 1), 0).astype(np.int64)
    return ds, L, A, D


def axis_nodes(c, p):
    """clearance_ref.axis_node for an array of coordinates: (lowest j minimising |p - c[j]| in fp32 after the clamp, outside flags)"""
    c = np.asarray(c, np.float32)
    p = np.asarray(p, np.float32).copy()
    lo, hi = c.min(), c.max()
    below = ~(p >= lo)
    above = ~below & (p > hi)
    p[below] = lo
    p[above] = hi
    j = np.empty(len(p), np.int64)
    for s in range(0, len(p), 1 << 16):
        q = p[s:s + (1 << 16)]
        j[s:s + len(q)] = np.argmin(np.abs(q[:, None] - c[None, :]), axis=1)
    return j, below | above


def sample_d2(grid, xyz):
    """(d2 of every sample's voxel, n_outside): the lookup of wa_traj_clearance; grid = (free, d2, dims, axes)"""
    _, d2, (nx, ny, nz), (cx, cy, cz) = grid
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    x, ox = axis_nodes(cx, xyz[:, 0])
    y, oy = axis_nodes(cy, xyz[:, 1])
    z, oz = axis_nodes(cz, xyz[:, 2])
    ids = (z * ny + y) * nx + x
    return np.asarray(d2, np.int32).ravel()[ids], int((ox | oy | oz).sum())


def caps(xyz, lim, v_limit=None, grid=None):
    """(C int64, kind uint8, n_outside) -- rule 2"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    vm = np.full(n, np.float64(lim["v_max"]))
    if v_limit is not None:
        vm = np.minimum(vm, np.asarray(v_limit, np.float32).astype(np.float64))
    cap = vm * vm
    kind = np.full(n, KIND_VMAX, np.uint8)
    a_lat = np.float64(lim["a_lat"])
    if n > 2 and np.isfinite(a_lat) and a_lat != 0.0:
        u, v, w = p[1:-1] - p[:-2], p[2:] - p[1:-1], p[2:] - p[:-2]
        cr = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        c = _norm(cr)
        den = (_norm(u) * _norm(v)) * _norm(w)
        ok = (c > 0) & (den > 0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            k2 = a_lat / ((np.float64(2.0) * c) / den)
        k2 = np.where(ok, k2, np.inf)
        take = k2 < cap[1:-1]
        cap[1:-1] = np.where(take, k2, cap[1:-1])
        kind[1:-1] = np.where(take, KIND_CURV, kind[1:-1])
    n_outside = 0
    if grid is not None:
        sd, n_outside = sample_d2(grid, xyz)
        if lim["near_d2"] >= 0:
            k3 = np.float64(lim["v_near"]) * np.float64(lim["v_near"])
            take = (sd <= lim["near_d2"]) & (k3 < cap)
            cap = np.where(take, k3, cap)
            kind = np.where(take, KIND_NEAR, kind).astype(np.uint8)
    cap[0] = cap[-1] = 0.0
    kind[0] = kind[-1] = KIND_END
    with np.errstate(over="ignore"):
        q = cap * QF
    big = ~(q < float(CAP_INF))
    C = np.where(big, CAP_INF, np.floor(np.where(big, 0.0, q)).astype(np.int64)).astype(np.int64)
    return C, kind, n_outside


def passes(C, A, D):
    """(F, B) by the closed forms of rule 3"""
    GA = np.concatenate([[0], np.cumsum(A)]).astype(np.int64)
    GD = np.concatenate([[0], np.cumsum(D)]).astype(np.int64)
    F = np.minimum.accumulate(C - GA) + GA
    B = np.minimum.accumulate((F + GD)[::-1])[::-1] - GD
    return F, B


def passes_sequential(C, A, D):
    """(F, B) by the recurrences of rule 3, one sample after the other (python integers)"""
    n = len(C)
    F = [0] * n
    B = [0] * n
    F[0] = int(C[0])
    for i in range(1, n):
        F[i] = min(int(C[i]), F[i - 1] + int(A[i - 1]))
    B[n - 1] = F[n - 1]
    for i in range(n - 2, -1, -1):
        B[i] = min(F[i], B[i + 1] + int(D[i]))
    return np.array(F, np.int64), np.array(B, np.int64)


def bound_bits(C, B, A, D, kind):
    """rule 4"""
    b = (B == C).astype(np.uint8)
    b[1:] |= ((B[1:] - B[:-1]) == A).astype(np.uint8) << 1
    b[:-1] |= ((B[:-1] - B[1:]) == D).astype(np.uint8) << 2
    return (b | (kind.astype(np.uint8) << 4)).astype(np.uint8)


def times(ds, L, B, acc, dec):
    """(dt float64, T int64, triangle mask, t_up float64) per segment -- rule 5"""
    acc, dec = np.float64(acc), np.float64(dec)
    v = np.sqrt(B.astype(np.float64) / QF)
    vs = v[:-1] + v[1:]
    tri = (L > 0) & (vs == 0)
    moving = (L > 0) & ~tri
    wp = (((np.float64(2.0) * ds) * acc) * dec) / (acc + dec)
    t_up = np.sqrt(wp) / acc
    dt_b = t_up + np.sqrt(wp) / dec
    with np.errstate(divide="ignore", invalid="ignore"):
        dt_c = (np.float64(2.0) * ds) / vs
    dt = np.where(tri, dt_b, np.where(moving, dt_c, 0.0))
    T = _quanta(dt)
    return dt, T, tri, t_up


def tick_count(time, tick_q):
    return time // tick_q + 1 + (1 if time % tick_q else 0)


def ticks(xyz, ds, L, B, dt, tri, t_up, time_q, tick_q, acc, dec):
    """the positions of rule 6 (float32 [n_ticks, 3])"""
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    n = len(p)
    time = int(time_q[-1])
    taus = np.arange(time // tick_q + 1, dtype=np.int64) * np.int64(tick_q)
    if time % tick_q:
        taus = np.concatenate([taus, [time]])
    i = np.searchsorted(time_q[:n - 1], taus, side="right") - 1
    e = (taus - time_q[i]).astype(np.float64) / QF
    acc, dec = np.float64(acc), np.float64(dec)
    v = np.sqrt(B.astype(np.float64) / QF)
    dsi = ds[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = ((B[i + 1] - B[i]).astype(np.float64) / QF) / (np.float64(2.0) * dsi)
        s_c = (v[i] * e) + ((np.float64(0.5) * a) * e) * e
        r = dt[i] - e
        s_b = np.where(e <= t_up[i], ((np.float64(0.5) * acc) * e) * e, dsi - ((np.float64(0.5) * dec) * r) * r)
        lam = np.where(tri[i], s_b, s_c) / dsi
    lam = np.where(lam < 0.0, 0.0, np.where(lam > 1.0, 1.0, lam))
    at_end = taus >= time_q[i + 1]
    still = L[i] == 0
    lam = np.where(at_end | still, 0.0, lam)
    out = (p[i] + (p[i + 1] - p[i]) * lam[:, None]).astype(np.float32)
    out[still & ~at_end] = p32[i[still & ~at_end]]
    out[at_end] = p32[i[at_end] + 1]
    return out


def retime(xyz, lim, v_limit=None, grid=None, tick=0.01, want_ticks=True):
    """the whole call: dict(time_q, w_q, bound, ticks, summary, ...); ValueError where the call answers WA_ERR_ARG"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    fin = lambda x: np.isfinite(x) and x > 0
    if n < 2 or not (fin(lim["v_max"]) and fin(lim["acc"]) and fin(lim["dec"])) or np.isnan(lim["a_lat"]) or lim["a_lat"] < 0:
        raise ValueError("limits")
    if grid is not None and lim["near_d2"] >= 0 and not fin(lim["v_near"]):
        raise ValueError("v_near")
    if v_limit is not None:
        v_limit = np.asarray(v_limit, np.float32)
        if len(v_limit) != n or not (np.isfinite(v_limit) & (v_limit > 0)).all():
            raise ValueError("v_limit")
    if not np.isfinite(xyz).all() or not np.isfinite(tick):
        raise ValueError("not finite")
    tq = np.rint(np.float64(tick) * QF)
    if not (tq >= 1 and tq <= float(CAP_INF)):
        raise ValueError("tick")
    tick_q = int(tq)
    ds, L, A, D = segments(xyz, lim["acc"], lim["dec"])
    for s in (L, A, D):
        if sum(int(x) for x in s[s >= (1 << 40)]) + int(s[s < (1 << 40)].sum()) >= CAP_INF:
            raise ValueError("sum reaches 2^61")
    C, kind, n_outside = caps(xyz, lim, v_limit, grid)
    F, B = passes(C, A, D)
    bound = bound_bits(C, B, A, D, kind)
    dt, T, tri, t_up = times(ds, L, B, lim["acc"], lim["dec"])
    if sum(int(x) for x in T[T >= (1 << 40)]) + int(T[T < (1 << 40)].sum()) >= CAP_INF:
        raise ValueError("duration reaches 2^61")
    time_q = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    time = int(time_q[-1])
    n_ticks = tick_count(time, tick_q)
    summary = dict(n=n, n_ticks=n_ticks, length_q=int(L.sum()), time_q=time,
                   n_bound=[int((kind == k).sum()) for k in range(4)],
                   n_on_cap=int((bound & 1).astype(bool).sum()), n_on_ramp=int((bound & 6).astype(bool).sum()),
                   n_triangle=int(tri.sum()), n_outside=int(n_outside), peak_w_q=int(B.max()))
    out = dict(time_q=time_q, w_q=B, bound=bound, summary=summary, C=C, F=F, A=A, D=D, L=L, ds=ds, kind=kind, T=T, tick_q=tick_q, ticks=None)
    if want_ticks and n_ticks <= MAX_TICKS:
        out["ticks"] = ticks(xyz, ds, L, B, dt, tri, t_up, time_q, tick_q, lim["acc"], lim["dec"])
    return out


# ------------------------------------------------------------------ scenes for the tests
def line(n, length=2.0):
    """n samples, evenly spaced in float64 and rounded to fp32, on a straight line of `length` along x"""
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = (np.arange(n, dtype=np.float64) * (length / (n - 1))).astype(np.float32)
    return xyz


def densify(points, per_leg):
    """every leg of a polyline cut into per_leg equal pieces (float64, rounded to fp32); corner points are kept exactly"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    out = [pts[:1]]
    t = (np.arange(1, per_leg + 1, dtype=np.float64) / per_leg)[:, None]
    for a, b in zip(pts[:-1], pts[1:]):
        out.append(a[None, :] + (b - a)[None, :] * t)
        out[-1][-1] = b
    return np.concatenate(out).astype(np.float32)


def right_angle(per_leg=200, leg=1.0):
    return densify([[0, 0, 0], [leg, 0, 0], [leg, leg, 0]], per_leg)


def helix(n, radius=0.5, pitch=0.05, turns=2.0):
    """n samples of a helix: constant curvature radius / (radius^2 + (pitch / 2 pi)^2)"""
    t = np.arange(n, dtype=np.float64) * (2.0 * np.pi * turns / (n - 1))
    return np.stack([radius * np.cos(t), radius * np.sin(t), pitch * t / (2.0 * np.pi)], 1).astype(np.float32)


def unit_axes(dims):
    return tuple(np.arange(k, dtype=np.float32) for k in dims)


def make_grid(free, dims, axes=None):
    """(free, d2, dims, axes) with the exact distance field of clearance_ref"""
    import clearance_ref as CR
    free = np.asarray(free, np.uint8).ravel()
    return free, CR.edt_separable(free, *dims), tuple(dims), unit_axes(dims) if axes is None else axes


def slab_scene(per_leg=150):
    """a 24 x 16 x 8 grid (unit axes) whose only metal is the slab x in 10..13, y in 0..5, all z; a straight pass along y = 8 at z = 4
    from x = 1 to x = 22: its samples over the slab are 3 voxels from the metal (d2 = 9), those far from it are not near"""
    dims = (24, 16, 8)
    free = np.ones(dims[::-1], np.uint8)   # [z, y, x]
    free[:, 0:6, 10:14] = 0
    return make_grid(free, dims), densify([[1, 8, 4], [22, 8, 4]], per_leg)


def random_scene(seed):
    """a seeded scene: an m^3 grid (16 .. 24, unit axes) with 1 - 3 % metal, a polyline of 4 - 9 random corner points inside it with
    3 - 60 samples per leg, a corner point now and then repeated; limits under which every kind of cap can bind; a per-sample limit for
    every second seed.  Returns (grid, xyz, limits, v_limit, tick)."""
    rs = np.random.RandomState(seed)
    m = int(rs.randint(16, 25))
    dims = (m, m, m)
    free = (rs.uniform(size=m ** 3) >= rs.uniform(0.01, 0.03)).astype(np.uint8)
    k = int(rs.randint(4, 10))
    corners = rs.uniform(1.0, m - 2.0, (k, 3))
    parts = [corners[:1].astype(np.float32)]
    for a, b in zip(corners[:-1], corners[1:]):
        leg = densify([a, b], int(rs.randint(3, 61)))[1:]
        parts.append(leg)
        if rs.uniform() < 0.3:
            parts.append(np.repeat(leg[-1:], int(rs.randint(1, 4)), 0))
    xyz = np.concatenate(parts).astype(np.float32)
    lim = limits(v_max=rs.uniform(0.5, 2.0), acc=rs.uniform(0.5, 4.0), dec=rs.uniform(0.5, 4.0), a_lat=rs.uniform(0.2, 2.0),
                 v_near=rs.uniform(0.1, 0.4), near_d2=int(rs.randint(1, 6)))
    v_limit = rs.uniform(0.2, 3.0, len(xyz)).astype(np.float32) if seed % 2 else None
    tick = float(rs.choice([0.004, 0.01, 0.05]))
    return make_grid(free, dims), xyz, lim, v_limit, tick


# Seeds for random_scene.  Chosen by running this file's retime() on the CPU over the candidate seeds 0 .. 23: for every candidate the
# kinds that bind somewhere (a sample with B == C whose cap has that kind) were listed; the condition is that each of the kinds 1, 2 and
# 3 binds on at least half of the kept scenes (kind 0 binds on every scene: the end points).  tests/test_retime_rules.py asserts it.
RANDOM_SEEDS = list(range(24))
