"""GPU tests of wa_traj_retime through the C ABI against tests/retime_ref.py (the header's definition in numpy), bit for bit: time_q_out,
w_q_out, bound_out, the tick positions and every field of the summary.

The scan works on tiles of 2 048 samples and gains a level at 2 049 and at 2^22 + 1 samples; a fourth level would begin at 2^33 + 1,
beyond the 2^31 samples the call accepts, so the sizes below cover every level there is."""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as CR
import fit_ref as F
import retime_ref as R
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def _same(ctx, xyz, lim, v_limit=None, grid=None, tick=0.01, g=None, traj=None):
    """one call against the reference: everything the call returns; returns (reference result, ticks Trajectory)"""
    r = R.retime(xyz, lim, v_limit, grid, tick)
    own_g = grid is not None and g is None
    if own_g:
        g = grid_of(ctx, grid)
    t = traj if traj is not None else api.Trajectory.from_points(ctx, xyz)
    time_q, w_q, bound, ticks, s = t.retime(lim["v_max"], lim["acc"], lim["dec"], tick, a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"],
                                            near_d2=lim["near_d2"], v_limit=v_limit)
    what = (len(xyz), lim, tick, grid is not None, v_limit is not None)
    assert s == r["summary"], (what, s, r["summary"])
    assert np.array_equal(w_q, r["w_q"]), (what, np.flatnonzero(w_q != r["w_q"])[:5])
    assert np.array_equal(bound, r["bound"]), (what, np.flatnonzero(bound != r["bound"])[:5])
    assert np.array_equal(time_q, r["time_q"]), (what, np.flatnonzero(time_q != r["time_q"])[:5])
    pts = ticks.points()
    assert pts.shape == r["ticks"].shape, what
    assert np.array_equal(bits(pts), bits(r["ticks"])), (what, np.flatnonzero((bits(pts) != bits(r["ticks"])).any(1))[:5])
    if traj is None:
        t.close()
    if own_g:
        g.close()
    return r, ticks


def test_hand_cases(ctx):
    lim = R.limits(v_max=0.5, acc=1, dec=2)
    r, _ = _same(ctx, R.line(100001), lim)                                                      # trapezoid
    assert abs(r["summary"]["time_q"] / R.Q - 4.375) < 1e-5
    r, _ = _same(ctx, R.line(1001, 0.1), lim)                                                   # triangle: v_max is not reached
    assert r["summary"]["peak_w_q"] < int(0.25 * R.Q)
    r, _ = _same(ctx, np.array([[0, 0, 0], [1, 2, 2]], np.float32), R.limits(v_max=9, acc=1, dec=3), tick=0.125)   # rule 5b
    assert r["summary"]["n_triangle"] == 1 and r["summary"]["n"] == 2
    _same(ctx, np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0]], np.float32), lim, tick=0.05)
    _same(ctx, np.zeros((5, 3), np.float32), lim)                                               # no length at all: one tick
    r, _ = _same(ctx, R.right_angle(), R.limits(v_max=1, acc=2, dec=2, a_lat=0.5))
    assert r["summary"]["n_bound"][2] >= 1
    r, _ = _same(ctx, R.right_angle(), R.limits(v_max=1, acc=2, dec=2, a_lat=np.inf))
    assert r["summary"]["n_bound"][2] == 0
    _same(ctx, R.right_angle(), R.limits(v_max=1, acc=2, dec=2, a_lat=0.0))
    r, _ = _same(ctx, R.helix(4001), R.limits(v_max=3, acc=5, dec=5, a_lat=0.4), tick=0.004)
    assert r["summary"]["n_bound"][2] > 3000
    _same(ctx, R.line(4001), lim, tick=2.0 ** -30 * 4096)                                        # ~2.9e5 ticks per second
    _same(ctx, R.line(11), lim, tick=100.0)                                                     # one tick period exceeds the duration


def test_slab_scene_near_the_metal(ctx):
    grid, xyz = R.slab_scene()
    lim = R.limits(v_max=2.0, acc=4.0, dec=4.0, v_near=0.25, near_d2=9)
    r, _ = _same(ctx, xyz, lim, grid=grid)
    assert r["summary"]["n_bound"][3] > 0
    on = (r["bound"] & 1).astype(bool) & (r["kind"] == 3)
    assert on.any() and (r["w_q"][on] == int(0.0625 * R.Q)).all()
    r, _ = _same(ctx, xyz, lim)                                                                 # g == NULL: no clearance cap
    assert r["summary"]["n_bound"][3] == 0
    lim["near_d2"] = -1
    r, _ = _same(ctx, xyz, lim, grid=grid)                                                      # grid given, cap switched off
    assert r["summary"]["n_bound"][3] == 0
    out = xyz.copy()
    out[:7, 1] = -3.0
    r, _ = _same(ctx, out, R.limits(v_max=2.0, acc=4.0, dec=4.0, v_near=0.25, near_d2=9), grid=grid)
    assert r["summary"]["n_outside"] == 7


def test_shuffled_axis_tables(ctx):
    """every other grid here has unit axes; clearance_ref's shuffled scene has a stretched x table, a shuffled y table (the lookup's
    scan) and a repeated last z node, and samples outside the tables' range"""
    free, dims, axes, xyz = CR.shuffled_scene()
    r, _ = _same(ctx, xyz, R.limits(v_max=2, acc=4, dec=4, v_near=0.25, near_d2=2), grid=R.make_grid(free, dims, axes), tick=0.01)
    assert r["summary"]["n_outside"] > 0 and r["summary"]["n_bound"][3] > 0


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_seeded_scenes(ctx, seed):
    grid, xyz, lim, v_limit, tick = R.random_scene(seed)
    g = grid_of(ctx, grid)
    _same(ctx, xyz, lim, v_limit, grid, tick, g=g)
    _same(ctx, xyz, lim, None, None, tick)
    other = np.random.RandomState(1000 + seed).uniform(0.2, 3.0, len(xyz)).astype(np.float32)
    _same(ctx, xyz, lim, other if v_limit is None else None, grid, tick, g=g)
    g.close()


@pytest.mark.parametrize("seed", F.RANDOM_SEEDS[:3])
def test_samples_of_the_trajectory_fit(ctx, seed):
    """the samples wa_grid_fit_trajectory returns for a seeded scene of fit_ref, re-timed as they lie on the device"""
    scene = F.random_scene(seed)
    free, d2, dims, axes, xyz = scene
    g = api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)
    poly = api.Trajectory.from_points(ctx, xyz)
    b, samples, _, _ = poly.fit(g, 3, F.RANDOM_SPACING, 6, F.RANDOM_SAMPLES)
    pts = samples.points()
    grid = (free, d2, dims, axes)
    lim = R.limits(v_max=3.0, acc=2.0, dec=2.5, a_lat=1.5, v_near=0.5, near_d2=2)
    vl = np.random.RandomState(seed).uniform(0.5, 4.0, len(pts)).astype(np.float32)
    for gr, gg in ((grid, g), (None, None)):
        for v in (None, vl):
            r, _ = _same(ctx, pts, lim, v, gr, 0.02, g=gg, traj=samples)
    assert len(samples.points()) == len(pts) and np.array_equal(bits(samples.points()), bits(pts))   # t is not modified
    for o in (samples, b, poly, g):
        o.close()


LEVEL_SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("n", LEVEL_SIZES)
def test_sizes_around_the_scan_levels(ctx, n):
    rs = np.random.RandomState(n)
    xyz = np.cumsum(rs.uniform(-0.01, 0.01, (n, 3)), 0).astype(np.float32)
    if n > 8:
        xyz[5] = xyz[4]
    _same(ctx, xyz, R.limits(v_max=0.3, acc=1.5, dec=0.7, a_lat=2.0), rs.uniform(0.05, 0.5, n).astype(np.float32), None, 0.01)


def _wavy(n):
    """n samples of a smooth curve with bends of every radius: curvature, v_limit and v_max all bind somewhere"""
    t = np.arange(n, dtype=np.float64) * (40.0 / n)
    return np.stack([t * 0.05, 0.3 * np.sin(t), 0.2 * np.cos(0.37 * t * t / 10.0)], 1).astype(np.float32)


@pytest.mark.parametrize("n", [(1 << 22) - 1, 1 << 22, (1 << 22) + 1])
def test_sizes_around_the_third_scan_level(ctx, n):
    r, _ = _same(ctx, _wavy(n), R.limits(v_max=0.8, acc=1.0, dec=1.5, a_lat=0.6), None, None, 0.001)
    assert min(r["summary"]["n_bound"][1:3]) > 0


def test_three_million_samples_with_a_grid(ctx):
    n = 3000000
    grid, _ = R.slab_scene()
    xyz = _wavy(n) * np.float32(8.0) + np.array([2.0, 8.0, 4.0], np.float32)
    vl = np.random.RandomState(5).uniform(0.5, 6.0, n).astype(np.float32)
    r, _ = _same(ctx, xyz, R.limits(v_max=4.0, acc=3.0, dec=3.0, a_lat=2.0, v_near=1.0, near_d2=16), vl, grid, 0.002)
    assert min(r["summary"]["n_bound"][1:]) > 0


def test_two_calls_give_the_same_bytes(ctx):
    grid, xyz, lim, v_limit, tick = R.random_scene(5)
    g = grid_of(ctx, grid)
    t = api.Trajectory.from_points(ctx, xyz)
    kw = dict(a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"], v_limit=v_limit)
    a = t.retime(lim["v_max"], lim["acc"], lim["dec"], tick, **kw)
    b = t.retime(lim["v_max"], lim["acc"], lim["dec"], tick, **kw)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3].points().tobytes() == b[3].points().tobytes() and a[4] == b[4]
    big = _wavy(300001)
    t2 = api.Trajectory.from_points(ctx, big)
    a = t2.retime(0.8, 1.0, 1.5, 0.001, a_lat=0.6)
    b = t2.retime(0.8, 1.0, 1.5, 0.001, a_lat=0.6)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3].points().tobytes() == b[3].points().tobytes() and a[4] == b[4]


def test_ticks_clear_the_grid_where_the_samples_do(ctx):
    """the slab scene's pass keeps 3 voxels from the metal: its samples hit nothing, and neither do the positions sent to the controller"""
    grid, xyz = R.slab_scene()
    g = grid_of(ctx, grid)
    t = api.Trajectory.from_points(ctx, xyz)
    assert t.clearance(g)[3]["n_hit"] == 0
    _, _, _, ticks, s = t.retime(2.0, 4.0, 4.0, 0.004, grid=g, v_near=0.25, near_d2=9)
    assert len(ticks) == s["n_ticks"] > 1000
    cs = ticks.clearance(g)[3]
    assert cs["n_hit"] == 0 and cs["n_outside"] == 0 and cs["min_d2"] == 9


def test_optional_outputs_and_capacity(ctx):
    lib = ctx.lib
    xyz = R.line(1001)
    t = api.Trajectory.from_points(ctx, xyz)
    lim = L.RetimeLimits(0.5, 1.0, 2.0, float("inf"), 0.0, -1)
    s = L.RetimeSummary()
    assert lib.wa_traj_retime(None, t.h, C.byref(lim), None, C.c_double(0.01), None, None, None, None, C.byref(s)) == 0
    r = R.retime(xyz, R.limits(v_max=0.5, acc=1, dec=2), tick=0.01)
    assert (s.time_q, s.n_ticks, s.length_q) == (r["summary"]["time_q"], r["summary"]["n_ticks"], r["summary"]["length_q"])
    # 4.4 s at a tick of one quantum: 4.7e9 ticks
    th = C.c_void_p(12345)
    w = np.zeros(len(xyz), np.int64)
    rc = lib.wa_traj_retime(None, t.h, C.byref(lim), None, C.c_double(2.0 ** -30), None, w.ctypes.data, None, C.byref(th), C.byref(s))
    assert rc == 7 and th.value is None and s.n_ticks == r["summary"]["time_q"] + 1 and np.array_equal(w, r["w_q"])


def test_every_argument_error_leaves_the_outputs_untouched(ctx):
    lib = ctx.lib
    grid, xyz = R.slab_scene(20)
    g = grid_of(ctx, grid)
    t = api.Trajectory.from_points(ctx, xyz)
    n = len(xyz)
    one = api.Trajectory.from_points(ctx, xyz[:1])
    nan = xyz.copy()
    nan[7, 1] = np.nan
    inf = xyz.copy()
    inf[0, 2] = np.inf
    far = xyz.copy()
    far[3, 0] = 3.0e38           # a segment of 3e38 units: L reaches 2^61
    slow = np.array([[0, 0, 0], [1.0e9, 0, 0]], np.float32)   # fits as a length, not as a time at 1e-10 units / s^2
    other = api.Context(0)
    og = grid_of(other, grid)
    good = dict(v_max=1.0, acc=1.0, dec=1.0, a_lat=float("inf"), v_near=0.5, near_d2=4)
    vl = np.full(n, 1.0, np.float32)

    def call(traj=t.h, grid_h=g.h, tick=0.01, v_limit=None, lim=True, summ=True, **kw):
        d = dict(good, **kw)
        lm = L.RetimeLimits(d["v_max"], d["acc"], d["dec"], d["a_lat"], d["v_near"], d["near_d2"])
        m = int(lib.wa_traj_size(traj)) if traj is not None else n
        tq, wq, bd = np.full(m, -7, np.int64), np.full(m, -7, np.int64), np.full(m, 0xAB, np.uint8)
        th, s = C.c_void_p(4242), L.RetimeSummary()
        s.n = -7
        s.time_q = -7
        rc = lib.wa_traj_retime(grid_h, traj, C.byref(lm) if lim else None, v_limit.ctypes.data if v_limit is not None else None,
                                C.c_double(tick), tq.ctypes.data, wq.ctypes.data, bd.ctypes.data, C.byref(th), C.byref(s) if summ else None)
        untouched = (tq == -7).all() and (wq == -7).all() and (bd == 0xAB).all() and th.value == 4242 and s.n == -7 and s.time_q == -7
        return rc, untouched

    assert call()[0] == 0 and not call()[1]
    bad_vl = [vl.copy() for _ in range(4)]
    bad_vl[0][3] = 0.0
    bad_vl[1][n - 1] = -1.0
    bad_vl[2][0] = np.nan
    bad_vl[3][5] = np.inf
    cases = [dict(traj=None), dict(lim=False), dict(summ=False), dict(grid_h=og.h), dict(traj=one.h),
             dict(v_max=0.0), dict(v_max=-1.0), dict(v_max=float("inf")), dict(v_max=float("nan")),
             dict(acc=1.0e12), dict(dec=1.0e12),          # the sum of A / of D alone reaches 2^61, L's does not
             dict(acc=0.0), dict(acc=float("inf")), dict(acc=float("nan")), dict(dec=0.0), dict(dec=-2.0), dict(dec=float("inf")),
             dict(a_lat=-1.0), dict(a_lat=float("nan")), dict(v_near=0.0), dict(v_near=float("nan")), dict(v_near=float("inf")),
             dict(tick=0.0), dict(tick=-1.0), dict(tick=float("nan")), dict(tick=float("inf")), dict(tick=2.0 ** -32), dict(tick=1.0e10)]
    cases += [dict(v_limit=v) for v in bad_vl]
    for kw in cases:
        rc, untouched = call(**kw)
        assert rc == 1 and untouched, kw
    for pts in (nan, inf, far):
        tr = api.Trajectory.from_points(ctx, pts)
        for gh in (g.h, None):
            rc, untouched = call(traj=tr.h, grid_h=gh)
            assert rc == 1 and untouched, pts[:8]
        tr.close()
    tr = api.Trajectory.from_points(ctx, slow)
    rc, untouched = call(traj=tr.h, grid_h=None, v_max=1.0e-9, acc=1.0e-10, dec=1.0e-10)
    assert rc == 1 and untouched
    tr.close()
    # what is NOT an error: v_near out of range while unused, a_lat 0 and +inf
    assert call(grid_h=None, v_near=float("nan"))[0] == 0 and call(near_d2=-1, v_near=-1.0)[0] == 0 and call(a_lat=0.0)[0] == 0
    for o in (og, t, one, g):
        o.close()
    other.close()
