"""numpy restatement of wa_grid_pose_fit_trajectory (include/weldacs.h, rules 37 - 39 of the torch section), written from the header's
definition and independent of the kernels: the loop of wa_grid_fit_trajectory with "a planned direction is open along this piece of
curve" in place of "this piece of curve is free".  Steps 1 - 3, 5 and 6 are fit_ref's functions, the spline is the oracle's, the voxel
lookup and the occupancy test are clearance_ref.clearance, the cover is clearance_ref.supercover, open(v, k) is reach_ref.open_dirs and
U is torch_ref.turn.  grid = (free, d2, dims, axes) as torch_ref.make_grid returns it.  No GPU, no product code."""
import numpy as np

import clearance_ref as CR
import fit_ref as F
import pose_ref as PR
import pose_shortcut_ref as PS
import reach_ref as RR
import torch_ref as TR

SUMMARY_FIELDS = ("rounds", "max_level_used", "n_legs", "n_legs_at_cap", "n_cps", "n_blocked_first", "n_blocked", "first_blocked",
                  "n_no_candidate", "n_dir_changes", "max_dir_turn")


def candidates(knots, n_cps, degree, own, holds, i, dt):
    """rule 37: the holds of the owners of control points span - D .. span, for the span of u_i, then of u_(i+1); -1 dropped, the first
    occurrence of each value kept"""
    out = []
    for e in (i, i + 1):
        span = F.find_span(knots, np.float32(e) * np.float32(dt))
        if span is None or span - degree < 0 or span >= n_cps:
            continue
        for c in range(span - degree, span + 1):
            h = int(holds[own[c]])
            if h >= 0 and h not in out:
                out.append(h)
    return out


def cover_ids(dims, a, b):
    """raster ids of the supercover between the voxels with ids a and b, voxel a included"""
    nx, ny, _ = dims
    vox = lambda v: (v % nx, (v // nx) % ny, v // (nx * ny))   # noqa: E731
    return np.array([(z * ny + y) * nx + x for x, y, z in CR.supercover(vox(int(a)), vox(int(b)))], np.int64)


def segment_test(opened, dims, ids, hits, knots, n_cps, degree, own, holds, dt):
    """rule 37 for every segment of one round: (seg_dir int32, blocked uint8, n_no_candidate)"""
    n_seg = len(ids) - 1
    seg_dir, blocked = np.full(n_seg, -1, np.int32), np.zeros(n_seg, np.uint8)
    n_none = 0
    for i in range(n_seg):
        cand = candidates(knots, n_cps, degree, own, holds, i, dt)
        if not cand:
            n_none += 1
            blocked[i] = hits[i]
            continue
        cover = cover_ids(dims, ids[i], ids[i + 1])
        for c in cand:
            if opened[cover, c].all():
                seg_dir[i] = c
                break
        else:
            blocked[i] = 1
    return seg_dir, blocked, n_none


def dir_stats(q, seg_dir):
    """(n_dir_changes, max_dir_turn) of rule 39"""
    d = np.asarray(seg_dir, np.int64)
    pair = (d[:-1] >= 0) & (d[1:] >= 0) & (d[:-1] != d[1:])
    if not pair.any():
        return 0, 0
    return int(pair.sum()), int(TR.turn(q[d[:-1][pair]], q[d[1:][pair]]).max())


def fit(grid, dirs, tool, xyz, holds, degree=3, spacing=1.0, max_level=6, n_samples=6001, opened=None, trace=None):
    """the whole call: dict(levels, knots, cps, samples, seg_dir, blocked, final, and SUMMARY_FIELDS)"""
    free, d2, dims, axes = grid
    nx, ny, nz = dims
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    holds = np.asarray(holds, np.int64).reshape(-1)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    n_legs = len(xyz) - 1
    assert n_legs >= 1 and len(holds) == n_legs and degree in (2, 3) and 0 <= max_level <= 8 and n_samples >= 2
    assert holds.min() >= -1 and holds.max() < len(dirs)
    if opened is None:
        opened = RR.open_dirs(grid, dirs, tool)
    q = TR.quantise_all(dirs)
    levels = np.zeros(n_legs, np.int32)
    out = {}
    for rnd in range(F.MAX_ROUNDS):
        m = F.pieces(xyz, levels, spacing)
        pts, leg = F.polygon(xyz, m)
        n_cps = len(pts) + 2 * (degree - 1)
        if n_cps > F.MAX_CPS:
            raise ValueError("more than 2^24 control points")
        b = F.fit_spline(pts, degree)
        dt = F.dt_of(F.fin_time_of(len(pts), degree), n_samples)
        samples, ok = b.sample(0.0, dt, n_samples)
        assert ok.all()
        ids, _, hits, summ = CR.clearance(free, d2, nx, ny, nz, axes[0], axes[1], axes[2], samples)
        own = F.owners(leg, degree)
        seg_dir, blocked, n_none = segment_test(opened, dims, ids, hits, b.knots, n_cps, degree, own, holds, dt)
        n_blocked = int(blocked.sum())
        if rnd == 0:
            out["n_blocked_first"] = n_blocked
        if trace is not None:
            trace.append(dict(n_cps=n_cps, n_blocked=n_blocked, levels=levels.copy()))
        out.update(rounds=rnd + 1, n_cps=n_cps, knots=b.knots, cps=b.cps, samples=samples, final=summ, levels=levels.copy(), dt=dt,
                   seg_dir=seg_dir, blocked=blocked, n_blocked=n_blocked, n_no_candidate=n_none, ids=ids, owners=own,
                   first_blocked=int(np.flatnonzero(blocked)[0]) if n_blocked else -1)
        mark = F.blame(b.knots, n_cps, degree, own, blocked, dt, n_legs)
        out["n_legs_at_cap"] = int((mark & (levels >= max_level)).sum())
        rise = mark & (levels < max_level)
        if n_blocked == 0 or not rise.any() or rnd == F.MAX_ROUNDS - 1:
            break
        levels[rise] += 1
    out["max_level_used"] = int(levels.max())
    out["n_legs"] = n_legs
    out["n_dir_changes"], out["max_dir_turn"] = dir_stats(q, out["seg_dir"])
    return out


def retest_plain_fit(grid, opened, xyz, holds, plain, degree, spacing):
    """the new segment test on what fit_ref.fit returned (`plain`): (seg_dir, blocked, n_no_candidate)"""
    _, leg = F.polygon(xyz, F.pieces(xyz, plain["levels"], spacing))
    free, d2, dims, axes = grid
    ids, _, hits, _ = CR.clearance(free, d2, *dims, *axes, plain["samples"])
    return segment_test(opened, dims, ids, hits, plain["knots"], plain["n_cps"], degree, F.owners(leg, degree), holds, plain["dt"])


# ------------------------------------------------------------------ scenes for the tests
def waypoints(grid, ids):
    """voxel centres (float32 [n, 3]) of the voxels `ids`"""
    _, _, (nx, ny, _), axes = grid
    ids = np.asarray(ids, np.int64)
    return np.stack([axes[0][ids % nx], axes[1][(ids // nx) % ny], axes[2][ids // (nx * ny)]], 1).astype(np.float32)


def _shortened(grid, dirs, tool, max_turn, ids, ks, opened, span=128):
    sc = PS.Scene(grid, dirs, tool, max_turn, opened)
    w, h, _ = sc.shortcut(ids, ks, span)
    return dict(grid=grid, dirs=np.asarray(dirs, np.float32).reshape(-1, 3), tool=tool, max_turn=max_turn, opened=opened,
                xyz=waypoints(grid, np.asarray(ids, np.int64)[w]), holds=h[:-1].astype(np.int32))


BOX_PAIRS = {1: (0, 2), 2: (0, 1), 3: (0, 4)}
_SCENES = {}


def scene(name):
    """a pose path shortened with span 128: dict(grid, dirs, tool, max_turn, opened, xyz, holds).  "pillars4", "pillars6" and "wide" are
    pose_shortcut_ref.scene_paths(); "box1", "box2", "box3" are pose_ref.box_case(seed)'s grid, directions and tool with max_turn
    250 000 and an unpinned path between two of its points (BOX_PAIRS).  Computed once per process, never modified."""
    if name not in _SCENES:
        if name.startswith("box"):
            seed = int(name[3:])
            c = PR.box_case(seed)
            sc = PR.Scene(c["grid"], c["dirs"], c["tool"], 250000)
            a, b = BOX_PAIRS[seed]
            hops, ids, ks = sc.path(c["points"][a], c["points"][b])
            assert hops >= 0
            _SCENES[name] = _shortened(c["grid"], c["dirs"], c["tool"], 250000, ids, ks, sc.opened)
        else:
            c = PS.scene_paths()[name]
            _SCENES[name] = _shortened(c["grid"], c["dirs"], c["tool"], c["max_turn"], c["ids"], c["ks"], c["opened"])
    return _SCENES[name]


_FITS = {}


def fitted(name, degree=3, spacing=8.0, max_level=6, n_samples=2001):
    """fit() of scene(name), computed once per process and parameter set, shared by the CPU and the GPU tests, never modified"""
    key = (name, degree, spacing, max_level, n_samples)
    if key not in _FITS:
        s = scene(name)
        _FITS[key] = fit(s["grid"], s["dirs"], s["tool"], s["xyz"], s["holds"], degree, spacing, max_level, n_samples, s["opened"])
    return _FITS[key]


def two_leg_case():
    """the candidate order by hand: a free 24 x 8 x 12 grid but for one voxel of metal above the middle of the second leg's row; the
    polyline (2, 4, 2) -> (10, 4, 2) -> (18, 4, 2) with holds [0, 1]; direction 0 points up (+z), direction 1 down (-z); the tool is a
    rod of 4 voxels.  Along the first leg both are open; under the metal voxel (14, 4, 5) direction 0 is closed and direction 1 open, so
    a segment there whose candidates are [0, 1] must take the second.  dict(grid, dirs, tool, xyz, holds)"""
    nx, ny, nz = 24, 8, 12
    free = np.ones((nz, ny, nx), np.uint8)
    free[5, 4, 14] = 0
    return dict(grid=TR.make_grid(free, (nx, ny, nz)), dirs=np.array([[0, 0, 1], [0, 0, -1]], np.float32), tool=TR.rod(4, 64, 0),
                xyz=np.array([[2, 4, 2], [10, 4, 2], [18, 4, 2]], np.float32), holds=np.array([0, 1], np.int32))
