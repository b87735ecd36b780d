"""numpy restatement of the torch-axis planner of include/weldacs.h (wa_traj_tool_axes, wa_traj_tool_check; rules 1 - 6), written from
the header's definition and independent of the kernels: python integers / int64 throughout.  It uses only a grid's occupancy, its
axis tables and the distance field of clearance_ref.py; grid = (free, d2, dims, axes) as retime_ref.make_grid returns it."""
import itertools

import numpy as np

import clearance_ref as CR

BLOCK = 1 << 36
INF = 1 << 62
D2_NONE = CR.D2_NONE
SUMMARY_FIELDS = ("n", "n_outside", "n_blocked_pairs", "n_no_dir", "n_chosen_blocked", "first_chosen_blocked", "n_chosen_near",
                  "n_over_turn", "max_turn_taken", "cost")


def unit_axes(dims):
    return tuple(np.arange(k, dtype=np.float32) for k in dims)


def make_grid(free, dims, axes=None):
    """(free, d2, dims, axes): free is [z, y, x] or flat in raster order, 1 = free"""
    free = np.asarray(free, np.uint8).ravel()
    return free, CR.edt_separable(free, *dims), tuple(dims), unit_axes(dims) if axes is None else axes


def weights(w_near=1, w_want=0, w_turn=1, near_add=-1, max_turn=-1):
    return dict(w_near=w_near, w_want=w_want, w_turn=w_turn, near_add=near_add, max_turn=max_turn)


# ---- rule 1
def quantise(v):
    """(q_x, q_y, q_z) of one float triple, or None when a component is not finite or the length is 0"""
    x, y, z = (np.float64(np.float32(c)) for c in v)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
        return None
    n = np.sqrt((x * x + y * y) + z * z)
    if not n > 0:
        return None
    return tuple(int(np.rint((c / n) * 16384.0)) for c in (x, y, z))


def quantise_all(dirs):
    q = [quantise(v) for v in np.asarray(dirs, np.float32).reshape(-1, 3)]
    if any(t is None for t in q):
        raise ValueError("a direction is not finite or has zero length")
    return np.array(q, np.int64).reshape(-1, 3)


def turn(a, b):
    """U(a, b), for arrays of triples that broadcast"""
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return (d * d).sum(-1) >> 10


# ---- rule 2
def offsets(q, dist16):
    """o[k, j, c] = floor((q[k, c] * dist16[j] + 2^17) / 2^18)"""
    q, dist16 = np.asarray(q, np.int64), np.asarray(dist16, np.int64)
    return (q[:, None, :] * dist16[None, :, None] + (1 << 17)) >> 18   # (>> on int64 is floor division)


def axis_nodes(c, p):
    """clearance_ref.axis_node for many coordinates: (node, outside)"""
    c = np.asarray(c, np.float32)
    p = np.asarray(p, np.float32).copy()
    lo, hi = c.min(), c.max()
    below = ~(p >= lo)
    above = ~below & (p > hi)
    p[below] = lo
    p[above] = hi
    return np.argmin(np.abs(p[:, None] - c[None, :]), axis=1).astype(np.int64), below | above


def sample_voxels(grid, xyz):
    _, _, _, (cx, cy, cz) = grid
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    x, ox = axis_nodes(cx, xyz[:, 0])
    y, oy = axis_nodes(cy, xyz[:, 1])
    z, oz = axis_nodes(cz, xyz[:, 2])
    return np.stack([x, y, z], 1), ox | oy | oz


def beads(grid, vox, off, r2, near_add):
    """vox: (..., 3) sample voxels, off: (..., n_beads, 3) offsets that broadcast against vox[..., None, :].  Returns (blocked, near) per
    bead as bool arrays: a bead outside the grid passes."""
    _, d2, (nx, ny, nz), _ = grid
    d2 = np.asarray(d2, np.int64).ravel()
    r2 = np.asarray(r2, np.int64)
    b = vox[..., None, :] + off
    inside = (b[..., 0] >= 0) & (b[..., 0] < nx) & (b[..., 1] >= 0) & (b[..., 1] < ny) & (b[..., 2] >= 0) & (b[..., 2] < nz)
    ids = np.where(inside, (b[..., 2] * ny + b[..., 1]) * nx + b[..., 0], 0)
    v = d2[ids]
    blocked = inside & (v <= r2)
    near = inside & ~blocked & (v <= r2 + near_add) if near_add >= 0 else np.zeros_like(blocked)
    return blocked, near


def feasibility(grid, xyz, q, tool, near_add):
    """(blocked bool[n, K], near int64[n, K], n_outside)"""
    dist16, r2 = tool
    vox, outside = sample_voxels(grid, xyz)
    off = offsets(q, dist16)                                   # K, n_beads, 3
    blocked = np.zeros((len(vox), len(q)), bool)
    near = np.zeros((len(vox), len(q)), np.int64)
    for s in range(0, len(vox), 256):
        b, m = beads(grid, vox[s:s + 256, None, :], off[None], r2, near_add)
        blocked[s:s + 256] = b.any(-1)
        near[s:s + 256] = m.sum(-1)
    return blocked, near, int(outside.sum())


# ---- rules 3 - 6
def wishes(want, n):
    """(qw int64[n, 3], given bool[n])"""
    qw, given = np.zeros((n, 3), np.int64), np.zeros(n, bool)
    if want is None:
        return qw, given
    want = np.asarray(want, np.float32).reshape(-1, 3)
    for i in range(n):
        if (want[i] == 0).all():
            continue
        t = quantise(want[i])
        if t is None:
            raise ValueError("a want entry is not finite")
        qw[i], given[i] = t, True
    return qw, given


def node_costs(blocked, near, q, qw, given, w):
    N = BLOCK * blocked.astype(np.int64) + w["w_near"] * near
    if given.any():
        N = N + np.where(given[:, None], w["w_want"] * turn(q[None, :, :], qw[:, None, :]), 0)
    return N


def transition(q, w):
    """T[k', k] = w_turn * U + BLOCK * [max_turn >= 0 and U > max_turn]"""
    U = turn(q[:, None, :], q[None, :, :])
    return w["w_turn"] * U + (BLOCK * (U > w["max_turn"]).astype(np.int64) if w["max_turn"] >= 0 else 0), U


def leg_sequence(N, T, pin_first, pin_last):
    """rule 5 for one leg with node costs N (len x K): (directions, cost)"""
    n, K = N.shape
    alpha = N[0].copy()
    if pin_first >= 0:
        keep = alpha[pin_first]
        alpha[:] = INF
        alpha[pin_first] = keep
    alpha = np.minimum(alpha, INF)
    back = np.zeros((n, K), np.int64)
    for i in range(1, n):
        cand = np.minimum(alpha[:, None] + T, INF)              # [k', k]
        back[i] = np.argmin(cand, axis=0)                       # the lowest k' among equals
        alpha = np.minimum(N[i] + cand[back[i], np.arange(K)], INF)
    last = pin_last if pin_last >= 0 else int(np.argmin(alpha))
    cost = int(alpha[last])
    seq = np.empty(n, np.int64)
    for i in range(n - 1, -1, -1):
        seq[i] = last
        last = back[i, last]
    return seq, cost


def plan(grid, xyz, dirs, tool, w, want=None, off=None, pin_first=None, pin_last=None):
    """wa_traj_tool_axes: dict(dir int32[n], feas uint8[n, K], leg_cost int64[n_legs], summary)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    q = quantise_all(dirs)
    K = len(q)
    off = np.asarray([0, n] if off is None else off, np.int64)
    n_legs = len(off) - 1
    blocked, near, n_outside = feasibility(grid, xyz, q, tool, w["near_add"])
    qw, given = wishes(want, n)
    N = node_costs(blocked, near, q, qw, given, w)
    T, U = transition(q, w)
    dirs_out = np.zeros(n, np.int32)
    leg_cost = np.zeros(n_legs, np.int64)
    n_over = max_taken = 0
    for l in range(n_legs):
        s, e = int(off[l]), int(off[l + 1])
        if s == e:
            continue
        seq, cost = leg_sequence(N[s:e], T, -1 if pin_first is None else int(pin_first[l]), -1 if pin_last is None else int(pin_last[l]))
        dirs_out[s:e], leg_cost[l] = seq, cost
        if e - s > 1:
            u = U[seq[:-1], seq[1:]]
            max_taken = max(max_taken, int(u.max()))
            if w["max_turn"] >= 0:
                n_over += int((u > w["max_turn"]).sum())
    idx = np.arange(n)
    ch_blocked = blocked[idx, dirs_out] if n else np.zeros(0, bool)
    ch_near = ~ch_blocked & (near[idx, dirs_out] > 0) if n else np.zeros(0, bool)
    cost = 0
    for c in leg_cost:
        if c < INF:
            cost = min(cost + int(c), INF)
    summary = dict(n=n, n_outside=n_outside, n_blocked_pairs=int(blocked.sum()), n_no_dir=int(blocked.all(1).sum()) if n else 0,
                   n_chosen_blocked=int(ch_blocked.sum()), first_chosen_blocked=int(np.flatnonzero(ch_blocked)[0]) if ch_blocked.any() else -1,
                   n_chosen_near=int(ch_near.sum()), n_over_turn=n_over, max_turn_taken=max_taken, cost=cost)
    feas = np.where(blocked, 255, near).astype(np.uint8)
    return dict(dir=dirs_out, feas=feas, leg_cost=leg_cost, summary=summary, N=N, T=T)


def check(grid, xyz, axes, tool, near_add):
    """wa_traj_tool_check: (blocked uint8[n], near uint8[n], summary)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    q = quantise_all(axes)
    dist16, r2 = tool
    vox, outside = sample_voxels(grid, xyz)
    off = offsets(q, dist16)                                   # n, n_beads, 3
    b, m = beads(grid, vox, off, r2, near_add)
    blocked, near = b.any(-1), m.sum(-1)
    nb = int(blocked.sum())
    summary = dict.fromkeys(SUMMARY_FIELDS, 0)
    summary.update(n=n, n_outside=int(outside.sum()), n_blocked_pairs=nb, n_no_dir=nb, n_chosen_blocked=nb,
                   first_chosen_blocked=int(np.flatnonzero(blocked)[0]) if nb else -1, n_chosen_near=int((~blocked & (near > 0)).sum()))
    return blocked.astype(np.uint8), near.astype(np.uint8), summary


def sequence_cost(N, T, seq, pin_first=-1, pin_last=-1):
    """the cost rule 5 gives ONE sequence (INF when it breaks a pin): what the exhaustive enumeration minimises"""
    if (pin_first >= 0 and seq[0] != pin_first) or (pin_last >= 0 and seq[-1] != pin_last):
        return INF
    c = int(N[0, seq[0]])
    for i in range(1, len(seq)):
        c = min(c + int(T[seq[i - 1], seq[i]]) + int(N[i, seq[i]]), INF)
    return c


def brute_force(N, T, pin_first=-1, pin_last=-1):
    """(optimum cost, every sequence attaining it) over all K^n sequences"""
    n, K = N.shape
    best, arg = None, []
    for seq in itertools.product(range(K), repeat=n):
        c = sequence_cost(N, T, seq, pin_first, pin_last)
        if best is None or c < best:
            best, arg = c, [seq]
        elif c == best:
            arg.append(seq)
    return best, arg


# ---- scenes
def densify(points, per_leg):
    pts = np.asarray(points, np.float64)
    out = [pts[:1]]
    for a, b in zip(pts[:-1], pts[1:]):
        t = np.arange(1, per_leg + 1)[:, None] / per_leg
        out.append(a + (b - a) * t)
    return np.concatenate(out).astype(np.float32)


def rod(n_beads, length16=16 * 12, r2=1):
    """a straight torch body: n_beads beads evenly spaced up to length16 sixteenths of a voxel behind the tip"""
    d = np.rint(np.linspace(0, length16, n_beads)).astype(np.int64) if n_beads > 1 else np.array([length16], np.int64)
    return d, np.full(n_beads, r2, np.int64)


def fib_dirs(K, half_angle=1.2, axis=(0.0, 0.0, 1.0)):
    """K directions on a cap around `axis` (direction 0 is the axis): the construction of api.torch_cone restated"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    helper = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(a, helper)
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    k = np.arange(K, dtype=np.float64)
    cos_t = 1.0 - (1.0 - np.cos(half_angle)) * (k / max(K - 1, 1))
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return (cos_t[:, None] * a + (sin_t * np.cos(phi))[:, None] * u + (sin_t * np.sin(phi))[:, None] * v).astype(np.float32)


def boxes_grid(rs, m, n_boxes):
    """an m^3 grid (unit axes) with n_boxes random boxes of metal"""
    free = np.ones((m, m, m), np.uint8)
    for _ in range(n_boxes):
        lo = rs.randint(0, m - 2, 3)
        sz = rs.randint(1, max(2, m // 4), 3)
        free[lo[2]:lo[2] + sz[2], lo[1]:lo[1] + sz[1], lo[0]:lo[0] + sz[0]] = 0
    return make_grid(free, (m, m, m))


def random_case(seed):
    """a seeded case: grid 24 .. 48 with random boxes, a polyline through it (a few samples outside the grid), K from the sizes at which
    k_torch_dp changes its block, 1 - 7 legs with empty ones, beads, weights, wishes and pins drawn.  Returns a dict of plan()'s arguments."""
    rs = np.random.RandomState(4000 + seed)
    m = int(rs.choice([24, 32, 48]))
    grid = boxes_grid(rs, m, int(rs.randint(3, 9)))
    corners = rs.uniform(-1.5 if seed % 5 == 0 else 1.0, m + (0.5 if seed % 5 == 0 else -2.0), (int(rs.randint(2, 7)), 3))
    xyz = densify(corners, int(rs.randint(2, 40)))
    n = len(xyz)
    K = int(rs.choice([1, 2, 3, 17, 63, 64, 65, 128, 255, 256]))
    dirs = fib_dirs(K, float(rs.uniform(0.4, 2.6)), rs.normal(size=3))
    nb = int(rs.choice([1, 5, 24, 33, 64]))
    tool = rod(nb, int(rs.randint(16, 16 * 14)), int(rs.randint(0, 6)))
    n_legs = int(rs.choice([1, 1, 2, 4, 7]))
    cuts = np.sort(rs.randint(0, n + 1, n_legs - 1)) if n_legs > 1 else np.zeros(0, np.int64)
    if n_legs >= 4:
        cuts[1] = cuts[0]                                      # an empty leg
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    w = weights(int(rs.randint(0, 1025)), int(rs.randint(0, 1025)), int(rs.randint(0, 1025)), int(rs.choice([-1, 0, 3, 20])),
                int(rs.choice([-1, -1, 1 << 14, 1 << 17])))
    want = None
    if seed % 3:
        want = rs.normal(size=(n, 3)).astype(np.float32)
        if seed % 3 == 1:
            want[rs.uniform(size=n) < 0.5] = 0
    pf = pl = None
    if seed % 2:
        pf = rs.randint(-1, K, n_legs).astype(np.int32)
        pl = rs.randint(-1, K, n_legs).astype(np.int32)
    return dict(grid=grid, xyz=xyz, dirs=dirs, tool=tool, w=w, want=want, off=off, pin_first=pf, pin_last=pl)


RANDOM_SEEDS = list(range(30))
