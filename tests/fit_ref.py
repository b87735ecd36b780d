"""numpy restatement of wa_grid_fit_trajectory (include/weldacs.h): steps 1, 2, 5 and 6 of the header's definition in numpy with
explicit float32 / float64 operations, steps 3 and 4 through the CPU oracle's spline (oracle_lib.Bspline, bit-equal to the kernels by
the existing goldens) and clearance_ref.clearance.  No GPU, no product code.

Every leg k has a level s_k, 0 at the start.  One round:
1. Pieces.  len_k = float64 length of leg k on the fp32 coordinates, sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded on its own;
   q = (len_k * 2^s_k) / (double)spacing; m_k = ceil(q) if ceil(q) >= 1 else 1.
2. Control polygon.  Leg k contributes j = 0 .. m_k - 1: per axis a + (b - a) * ((float)j / (float)m_k) in fp32; after the last leg,
   the last point.  Point 0 is the initial position, the last point the final position, the points between are the middle points.
   owner[c] = the leg a control point came from; the constrained control points at either end belong to the first / last leg.
3. Fit.  BS_Basic<float, 3, D, D-1, D-1>, zero end derivatives, fin_time = (float)(number of knot spans) = middle points + D.
4. Sample and check.  u_i = (float)i * dt, dt = fin_time / (float)(n_samples - 1); wa_traj_clearance's lookup and segment test.
5. Blame.  For a hit segment i, the knot spans of u_i and u_(i+1) (_findSpan); control points span - D .. span; their owners are marked.
6. Refine.  Marked legs below max_level rise by one.  Stop when no segment hit, no level changed, or after 32 rounds (the 32nd raises
   nothing)."""
import numpy as np

import clearance_ref as CR
import oracle_lib as O

MAX_ROUNDS = 32
MAX_CPS = 1 << 24


def leg_lengths(xyz):
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    d = p[1:] - p[:-1]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def pieces(xyz, levels, spacing):
    """m_k (int64) for every leg"""
    q = (leg_lengths(xyz) * np.float64(2.0) ** np.asarray(levels, np.int64)) / np.float64(np.float32(spacing))
    c = np.ceil(q)
    return np.where(c >= 1.0, c, 1.0).astype(np.int64)


def polygon(xyz, m):
    """(points float32 [sum m + 1, 3], leg of every point)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    m = np.asarray(m, np.int64)
    first = np.concatenate([[0], np.cumsum(m)])               # the first point of every leg
    leg = np.repeat(np.arange(len(m), dtype=np.int64), m)
    t = (np.arange(first[-1], dtype=np.int64) - first[leg]).astype(np.float32) / m[leg].astype(np.float32)
    step = (xyz[1:] - xyz[:-1]).astype(np.float32)
    pts = (xyz[leg] + (step[leg] * t[:, None]).astype(np.float32)).astype(np.float32)
    return np.concatenate([pts, xyz[-1:]]), np.concatenate([leg, [len(m) - 1]])


def owners(leg, degree):
    """owner of every control point: D - 1 constrained ones behind the first and before the last"""
    return np.concatenate([np.full(degree - 1, leg[0], np.int64), leg, np.full(degree - 1, leg[-1], np.int64)])


def fin_time_of(n_points, degree):
    return np.float32(n_points - 2 + degree)


def fit_spline(points, degree):
    """the oracle's BS_Basic<float, 3, D, D-1, D-1> on polygon `points` (steps 3)"""
    n_middle = len(points) - 2
    b = O.Bspline(3, degree, degree - 1, degree - 1, n_middle)
    z = np.zeros((degree - 1, 3), np.float32)
    b.set_param(np.vstack([points[:1], z]), np.vstack([points[-1:], z]), points[1:-1], fin_time_of(len(points), degree))
    return b


def dt_of(fin_time, n_samples):
    return np.float32(fin_time) / np.float32(n_samples - 1)


def find_span(K, u):
    """_findSpan (BSplineBasic.h:358-385) after the evaluation's clamp of u into the knot range; None where it refuses"""
    K = np.asarray(K, np.float32)
    u = np.float32(u)
    nk = len(K)
    if u < K[0]:
        u = K[0]
    elif u > K[-1]:
        u = K[-1]
    dd = np.float32(u - K[-1])
    if float(np.float32(dd * dd)) < 1.e-10:
        for i in range(nk - 2, -1, -1):
            if K[i] < u and u <= K[i + 1]:
                return i
        return None
    low, high = 0, nk - 1
    mid = (low + high) >> 1
    while u < K[mid] or u >= K[mid + 1]:
        if u < K[mid]:
            high = mid
        else:
            low = mid
        mid = (low + high) >> 1
    return mid


def blame(K, n_cps, degree, own, hits, dt, n_legs):
    mark = np.zeros(n_legs, bool)
    for i in np.flatnonzero(hits):
        for e in (i, i + 1):
            span = find_span(K, np.float32(e) * np.float32(dt))
            if span is None or span - degree < 0 or span >= n_cps:
                continue
            mark[own[span - degree:span + 1]] = True
    return mark


def fit(free, d2, dims, axes, xyz, degree=3, spacing=1.0, max_level=6, n_samples=6001, trace=None):
    """the whole call: dict(levels, rounds, n_cps, knots, cps, samples, n_hit_first, n_legs_at_cap, max_level_used, final)"""
    nx, ny, nz = dims
    cx, cy, cz = axes
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_legs = len(xyz) - 1
    assert n_legs >= 1 and degree in (2, 3) and 0 <= max_level <= 8 and n_samples >= 2
    levels = np.zeros(n_legs, np.int32)
    out = {}
    for rnd in range(MAX_ROUNDS):
        m = pieces(xyz, levels, spacing)
        pts, leg = polygon(xyz, m)
        n_cps = len(pts) + 2 * (degree - 1)
        if n_cps > MAX_CPS:
            raise ValueError("more than 2^24 control points")
        b = fit_spline(pts, degree)
        ft = fin_time_of(len(pts), degree)
        dt = dt_of(ft, n_samples)
        samples, ok = b.sample(0.0, dt, n_samples)
        assert ok.all()
        _, _, hits, summ = CR.clearance(free, d2, nx, ny, nz, cx, cy, cz, samples)
        if rnd == 0:
            out["n_hit_first"] = summ["n_hit"]
        if trace is not None:
            trace.append(dict(n_cps=n_cps, n_hit=summ["n_hit"], levels=levels.copy()))
        knots, cps = b.knots, b.cps
        out.update(rounds=rnd + 1, n_cps=n_cps, knots=knots, cps=cps, samples=samples, final=summ, levels=levels.copy(), polygon=pts,
                   fin_time=ft, dt=dt, hits=hits)
        mark = blame(knots, n_cps, degree, owners(leg, degree), hits, dt, n_legs)
        out["n_legs_at_cap"] = int((mark & (levels >= max_level)).sum())
        rise = mark & (levels < max_level)
        if summ["n_hit"] == 0 or not rise.any() or rnd == MAX_ROUNDS - 1:
            break
        levels[rise] += 1
    out["max_level_used"] = int(levels.max())
    out["n_legs"] = n_legs
    return out


# ------------------------------------------------------------------ scenes for the tests
def unit_axes(dims):
    return tuple(np.arange(n, dtype=np.float32) for n in dims)


def scene(free, dims, xyz, axes=None):
    """(free, d2, dims, axes, xyz) ready for fit()"""
    free = np.asarray(free, np.uint8).ravel()
    return free, CR.edt_separable(free, *dims), dims, unit_axes(dims) if axes is None else axes, np.asarray(xyz, np.float32).reshape(-1, 3)


def straight():
    """a straight polyline of three legs (the middle one of zero length) through a free 16 x 16 x 8 grid"""
    dims = (16, 16, 8)
    return scene(np.ones(16 * 16 * 8, np.uint8), dims, [[1, 2, 1], [5, 4, 2], [5, 4, 2], [13, 8, 4]])


def l_corner(long=False):
    """16 x 16 x 1, unit axes, the only occupied voxel (9, 3) inside the corner of the polyline (2, 2) -> (10, 2) -> (10, 10): the
    polyline's own voxels (row y = 2, column x = 10) are free, and a uniform cubic on control points 8 apart passes the corner
    8 / 6 = 1.33 voxels inside it, through (9, 3); 4 apart still 0.67 inside (x < 9.5 and y > 2.5); 2 apart it stays in row 2 and
    column 10.  At spacing 8 the corner therefore needs level 2.  long=True: the same corner inside a polyline of 7 legs."""
    dims = (16, 16, 1)
    free = np.ones(256, np.uint8)
    free[3 * 16 + 9] = 0
    xyz = [[2, 2, 0], [10, 2, 0], [10, 10, 0]] if not long else \
        [[2, 0, 0], [2, 2, 0], [6, 2, 0], [10, 2, 0], [10, 6, 0], [10, 10, 0], [12, 10, 0], [12, 14, 0]]
    return scene(free, dims, xyz)


def diagonal_graze():
    """the documented limit: the straight polyline (0, 0) -> (3, 3) steps from voxel (1, 1) to voxel (2, 2) through their shared corner
    (x and y cross 1.5 in the same sample pair, the curve being x == y exactly); the segment test then covers the whole product set,
    which holds the occupied (2, 1).  No spacing changes which voxels the line visits: every level is blamed, up to the cap."""
    dims = (16, 16, 1)
    free = np.ones(256, np.uint8)
    free[1 * 16 + 2] = 0
    return scene(free, dims, [[0, 0, 0], [3, 3, 0]])


def random_scene(seed):
    """a seeded scene: an n^3 grid (24..40, unit axes) with 5-15 % obstacles, a shortest lattice path between two far free voxels
    (geodesic_ref.paths) shortened by line of sight (shortcut_ref.shortcut); returns (free, d2, dims, axes, polyline xyz) or None when
    the two voxels are not connected"""
    import geodesic_ref as GR
    import shortcut_ref as SR
    rs = np.random.RandomState(seed)
    n = int(rs.randint(24, 41))
    occ = rs.uniform(0.05, 0.15)
    dims = (n, n, n)
    free = (rs.uniform(size=n ** 3) >= occ).astype(np.uint8)
    fr = np.flatnonzero(free)
    lo = fr[fr < n ** 3 // 8]
    hi = fr[fr >= n ** 3 - n ** 3 // 8]
    s, e = int(lo[rs.randint(len(lo))]), int(hi[rs.randint(len(hi))])
    hops, ps = GR.paths(free, dims, [s], [e])
    if ps[0] is None:
        return None
    axes = unit_axes(dims)
    w, _ = SR.shortcut(free, n, n, axes[0], axes[1], axes[2], ps[0], 128)
    ids = np.asarray(ps[0], np.int64)[w]
    xyz = np.stack([axes[0][ids % n], axes[1][(ids // n) % n], axes[2][ids // (n * n)]], 1).astype(np.float32)
    return scene(free, dims, xyz, axes)


# Seeds for random_scene, fitted at RANDOM_SPACING voxels (at one voxel the unrefined cubic already clears these scenes: the loop
# would have nothing to do).  Chosen by running this file's fit() on the CPU: the 40 candidate seeds 0 .. 39 were tried (cubic, max_level 6,
# 2001 samples); every one was connected and none had to be dropped for not reaching final.n_hit == 0.  19 of the 40 hit in round 1; the
# list keeps those 19 and the first 5 that do not.
RANDOM_SPACING = 8.0
RANDOM_SAMPLES = 2001
RANDOM_SEEDS = [0, 2, 4, 6, 9, 14, 15, 16, 19, 21, 23, 26, 27, 30, 31, 32, 34, 35, 39, 1, 3, 5, 7, 8]


# ------------------------------------------------------------------ polylines of many legs: the scan of the piece counts beyond one block
def _serpentine(n):
    """corner points of a boustrophedon through the voxels 1 .. n - 2 of an n^3 grid: rows along x one voxel apart in y, layers one voxel
    apart in z; it never comes back to a voxel it has left"""
    lo, hi = 1.0, float(n - 2)
    out = []
    fx = fy = True
    for z in range(1, n - 1):
        for y in (range(1, n - 1) if fy else range(n - 2, 0, -1)):
            out.append((lo if fx else hi, y, z))
            out.append((hi if fx else lo, y, z))
            fx = not fx
        fy = not fy
    return np.array(out, np.float64)


def many_legs_scene(n_legs, marks=(), seed=0, unit=1.0, zero_from=None, long_every=0, long_len=0.0):
    """(free, d2, dims, axes, xyz) with exactly n_legs legs: polyline points at growing arc length along a serpentine through a 48^3 grid
    (64^3 where 48^3 is too short for it), unit axes.  Leg k is `unit` times a length uniform in 0.05 .. 2.2 (at spacing == unit: m_k in
    1, 2, 3, differing between neighbours); about 2 % of the legs, in runs of 1 .. 5, have zero length (both ends the same fp32 point).
    zero_from: every leg from that index on has zero length.  long_every / long_len: every long_every-th leg (not leg 0) is long_len
    long instead.  The grid is free except for the voxel of polyline point k (the first point of leg k) for every k in marks: the
    control polygon keeps a point inside the metal there at every level, so the legs around k are blamed until they reach the cap."""
    rs = np.random.RandomState(seed)
    ln = rs.uniform(0.05, 2.2, n_legs) * unit
    k = 0
    while k < n_legs:                                           # runs of zero-length legs: 0.7 % starts x 3 legs on average
        if rs.uniform() < 0.007:
            run = int(rs.randint(1, 6))
            ln[k:k + run] = 0.0
            k += run
        k += 1
    if long_every:
        ln[long_every::long_every] = long_len
    if zero_from is not None:
        ln[zero_from:] = 0.0
    s = np.concatenate([[0.0], np.cumsum(ln)])
    for n in (48, 64):
        corners = _serpentine(n)
        at = np.concatenate([[0.0], np.cumsum(np.abs(np.diff(corners, axis=0)).sum(1))])
        if s[-1] <= at[-1]:
            break
    assert s[-1] <= at[-1], "the polyline does not fit into the grid"
    xyz = np.stack([np.interp(s, at, corners[:, c]) for c in range(3)], 1).astype(np.float32)
    assert len(xyz) == n_legs + 1
    dims = (n, n, n)
    axes = unit_axes(dims)
    free = np.ones(n ** 3, np.uint8)
    for k in marks:
        x, y, z = (CR.axis_node(axes[c], xyz[k, c])[0] for c in range(3))
        free[(z * n + y) * n + x] = 0
    return scene(free, dims, xyz, axes)


def block_marks(n_legs):
    """the legs the block tests mark: either side of a wave's and a block's edge, and the last leg"""
    return sorted({k for k in (0, 63, 64, 255, 256, 257, 511, 512, n_legs - 1) if k < n_legs})


def pass_marks(n_legs):
    """the legs the scan-pass tests mark: block_marks, either side of the 65 536th leg (256 blocks of 256: where k_fit_scan_sums starts
    its second trip), of the block behind it and of the third trip, and the last leg"""
    return sorted({k for k in (0, 63, 64, 255, 256, 257, 65535, 65536, 65537, 65792, 131071, 131072, n_legs - 1) if k < n_legs})


# Leg counts around one block of 256 legs (spacing 1, max_level 2, BLOCK_SAMPLES samples) and around one trip of 256 blocks (spacing 1,
# max_level 1, about as many samples as legs, so that a sample segment stays local and the blame does not creep).
# CPU time of the reference, fit() alone, as tests/test_fit_rules.py prints it: 0.3 to 0.5 s for every entry of BLOCK_LEGS and degree
# (3 rounds each), 0.6 s for "zero_tail" (3 rounds), 1.6 s for "long_legs" (10 rounds); 7.9, 7.0, 7.2, 6.7 and 14.5 s for the five
# entries of PASS_LEGS (2 rounds each: round 1 hits at every mark, round 2 finds the same legs at the cap and raises nothing).
BLOCK_LEGS = [63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
BLOCK_SAMPLES = 3001
PASS_LEGS = [65535, 65536, 65537, 65793, 131073]          # 131 073: a third trip of the block-sum scan
_many = {}


def many_legs_case(name, degree=3):
    """(scene, (degree, spacing, max_level, n_samples), reference result) of a named many-legs case; computed once per process, shared
    by tests/test_fit_rules.py and tests/test_gpu_fit.py, never modified"""
    key = (name, degree)
    if key not in _many:
        if name == "zero_tail":            # every leg behind the first 300 has zero length: m_k = 1, off[k] = k, one leg per emit lane
            n_legs = 1500
            sc = many_legs_scene(n_legs, [0, 100, 299, 300, n_legs - 1], 5, zero_from=300)
            par = (degree, 1.0, 2, BLOCK_SAMPLES)
        elif name == "long_legs":          # seven legs of up to 40 voxels (m_k = 400 .. 4000 at spacing 0.01) between stretches of m_k in 1, 2, 3
            n_legs = 700
            sc = many_legs_scene(n_legs, [0, 96, 97, 98, 300, 388, 389, n_legs - 1], 6, unit=0.01, long_every=97, long_len=40.0)
            par = (degree, 0.01, 2, BLOCK_SAMPLES)
        elif name < 65535:
            sc = many_legs_scene(name, block_marks(name), name)
            par = (degree, 1.0, 2, BLOCK_SAMPLES)
        else:
            sc = many_legs_scene(name, pass_marks(name), name)
            par = (degree, 1.0, 1, name + 4464)
        import time
        t0 = time.process_time()
        r = fit(*sc, *par)
        r["cpu_seconds"] = time.process_time() - t0
        _many[key] = (sc, par, r)
    return _many[key]
