"""GPU tests of the torch-axis planner (wa_traj_tool_axes, wa_traj_tool_check; Trajectory.torch_axes / torch_check) against
tests/torch_ref.py, the header's definition in numpy, bit for bit: dir_out, feas_out, leg_cost, every field of the summary, and the
check's outputs.

Sizes: k_torch_dp runs K rounded up to whole wavefronts (64, 128, 192, 256 threads), so K sits on and around those; k_torch_nodes takes
tiles of 32 samples and lays (sample, direction) pairs over 256 threads, so sample counts sit around 32 and K around 64 and 256; its
offsets need more than 64 KiB of LDS from K * n_beads > 8192 on (K = 256 with 33 and 64 beads)."""
import ctypes as C

import numpy as np
import pytest

import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG, CAPACITY = 1, 7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


@pytest.fixture(scope="module")
def boxes32(ctx):
    """one 32^3 grid with random boxes, shared: (reference grid, device grid)"""
    grid = T.boxes_grid(np.random.RandomState(7), 32, 8)
    g = grid_of(ctx, grid)
    yield grid, g
    g.close()


def _same(ctx, grid, xyz, dirs, tool, w, want=None, off=None, pin_first=None, pin_last=None, g=None, check=True):
    """one call against the restatement: everything it returns; then the chosen axes through the check.  Returns the reference result."""
    r = T.plan(grid, xyz, dirs, tool, w, want, off, pin_first, pin_last)
    own = g is None
    if own:
        g = grid_of(ctx, grid)
    t = api.Trajectory.from_points(ctx, xyz)
    o = t.torch_axes(g, dirs, tool, want=want, off=off, pin_first=pin_first, pin_last=pin_last, **w)
    what = (len(xyz), len(dirs), len(tool[0]), w, want is not None, None if off is None else list(off))
    assert np.array_equal(o["feas"], r["feas"]), (what, np.argwhere(o["feas"] != r["feas"])[:5])
    assert np.array_equal(o["leg_cost"], r["leg_cost"]), (what, o["leg_cost"], r["leg_cost"])
    assert np.array_equal(o["dir"], r["dir"]), (what, np.flatnonzero(o["dir"] != r["dir"])[:5])
    assert o["summary"] == r["summary"], (what, o["summary"], r["summary"])
    if check and len(xyz):
        axes = np.asarray(dirs, np.float32).reshape(-1, 3)[r["dir"]]
        cb, cn, cs = T.check(grid, xyz, axes, tool, w["near_add"])
        b, nr, s = t.torch_check(g, axes, tool, w["near_add"])
        assert np.array_equal(b, cb) and np.array_equal(nr, cn) and s == cs, (what, s, cs)
        assert s["n_chosen_blocked"] == r["summary"]["n_chosen_blocked"] and s["n_chosen_near"] == r["summary"]["n_chosen_near"]
    t.close()
    if own:
        g.close()
    return r


def _polyline(rs, m, n, lo=1.0):
    k = max(2, n // 25 + 2)
    xyz = T.densify(rs.uniform(lo, m - 1.0 - lo, (k, 3)), n // (k - 1) + 1)[:n]
    assert len(xyz) == n
    return xyz


LEGS7 = np.cumsum([0, 0, 1, 2, 63, 0, 64, 65])          # 7 legs, two of them empty: lengths 0, 1, 2, 63, 0, 64, 65


@pytest.mark.parametrize("K,n_beads", [(1, 33), (2, 64), (63, 1), (64, 33), (65, 64), (128, 1), (255, 33), (256, 64), (256, 33)])
def test_direction_counts_beads_and_legs(ctx, boxes32, K, n_beads):
    grid, g = boxes32
    rs = np.random.RandomState(K * 100 + n_beads)
    xyz = _polyline(rs, 32, int(LEGS7[-1]))
    dirs = T.fib_dirs(K, 2.2, (0.2, -0.3, 1.0))
    want = rs.normal(size=(len(xyz), 3)).astype(np.float32)
    want[::3] = 0
    pf, pl = rs.randint(-1, K, 7).astype(np.int32), rs.randint(-1, K, 7).astype(np.int32)
    w = T.weights(3, 2, 5, 6, 1 << 17)
    r = _same(ctx, grid, xyz, dirs, T.rod(n_beads, 16 * 9, 2), w, want, LEGS7, pf, pl, g=g)
    assert r["summary"]["n_blocked_pairs"] > 0 or K < 3
    _same(ctx, grid, xyz, dirs, T.rod(n_beads, 16 * 9, 2), T.weights(3, 2, 5, -1, -1), None, None, None, None, g=g, check=False)   # one leg, no pins


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97])
def test_sample_counts_around_the_tile(ctx, boxes32, n):
    grid, g = boxes32
    xyz = _polyline(np.random.RandomState(n), 32, n)
    for K in (17, 64):
        _same(ctx, grid, xyz, T.fib_dirs(K, 1.5), T.rod(5, 16 * 7, 1), T.weights(1, 0, 4, 3), g=g, check=K == 17)


def test_one_long_leg(ctx):
    rs = np.random.RandomState(11)
    grid = T.boxes_grid(rs, 48, 10)
    xyz = _polyline(rs, 48, 3001)
    r = _same(ctx, grid, xyz, T.fib_dirs(64, 1.3), T.rod(24, 16 * 12, 2), T.weights(2, 0, 1, 8, 1 << 16))
    assert r["summary"]["n_blocked_pairs"] > 0 and len(set(r["dir"])) > 3


def test_grid_without_obstacles_and_a_sample_inside_the_metal(ctx, boxes32):
    empty = T.make_grid(np.ones((24, 24, 24), np.uint8), (24, 24, 24))
    xyz = _polyline(np.random.RandomState(3), 24, 70)
    r = _same(ctx, empty, xyz, T.fib_dirs(65, 1.0), T.rod(33, 16 * 30, 1 << 30), T.weights(7, 0, 1, 1 << 30))
    assert r["summary"]["n_blocked_pairs"] == 0 and r["summary"]["n_chosen_near"] == 70          # WA_D2_NONE <= 2^30 + 2^30, by the letter
    r = _same(ctx, empty, xyz, T.fib_dirs(65, 1.0), T.rod(33, 16 * 30, 1 << 30), T.weights(7, 0, 1, 5))
    assert r["summary"]["n_chosen_near"] == 0
    grid, g = boxes32
    metal = np.flatnonzero(grid[0] == 0)[40]
    xyz = _polyline(np.random.RandomState(4), 32, 40)
    xyz[17] = [metal % 32, (metal // 32) % 32, metal // 1024]
    r = _same(ctx, grid, xyz, T.fib_dirs(64, 1.5), T.rod(5, 16 * 4, 0), T.weights(1, 0, 1), g=g)   # bead 0 sits on the tip: d2 = 0 <= 0
    assert r["summary"]["n_no_dir"] >= 1 and r["summary"]["n_chosen_blocked"] >= 1 and r["summary"]["first_chosen_blocked"] <= 17
    assert (r["feas"][17] == 255).all()


def test_samples_outside_the_grid(ctx, boxes32):
    grid, g = boxes32
    xyz = T.densify([[-4, 5, 5], [12, 12, 40], [36, 20, 3]], 30)
    r = _same(ctx, grid, xyz, T.fib_dirs(64, 2.8), T.rod(24, 16 * 10, 1), T.weights(1, 0, 1, 4), g=g)
    assert r["summary"]["n_outside"] > 10


@pytest.mark.parametrize("seed", T.RANDOM_SEEDS)
def test_seeded_cases(ctx, seed):
    c = T.random_case(seed)
    _same(ctx, c["grid"], c["xyz"], c["dirs"], c["tool"], c["w"], c["want"], c["off"], c["pin_first"], c["pin_last"])


def test_same_bytes_on_a_second_call(ctx, boxes32):
    grid, g = boxes32
    xyz = _polyline(np.random.RandomState(5), 32, 200)
    t = api.Trajectory.from_points(ctx, xyz)
    kw = dict(want=np.tile(np.float32([0, 1, 1]), (200, 1)), off=[0, 50, 50, 200], w_near=3, w_want=1, w_turn=2, near_add=5, max_turn=1 << 16)
    a = t.torch_axes(g, T.fib_dirs(128, 2.0), T.rod(24, 16 * 9, 2), **kw)
    b = t.torch_axes(g, T.fib_dirs(128, 2.0), T.rod(24, 16 * 9, 2), **kw)
    assert a["dir"].tobytes() == b["dir"].tobytes() and a["feas"].tobytes() == b["feas"].tobytes()
    assert a["leg_cost"].tobytes() == b["leg_cost"].tobytes() and a["summary"] == b["summary"]
    assert np.array_equal(t.points().view(np.uint32), xyz.view(np.uint32))                       # t is not modified
    t.close()


def test_refusals_leave_outputs_untouched(ctx, boxes32):
    grid, g = boxes32
    n, K = 40, 8
    xyz = _polyline(np.random.RandomState(6), 32, n)
    t = api.Trajectory.from_points(ctx, xyz)
    bad_xyz = xyz.copy()
    bad_xyz[7, 1] = np.nan
    nan = api.Trajectory.from_points(ctx, bad_xyz)
    bad_xyz[7, 1] = np.inf
    inf = api.Trajectory.from_points(ctx, bad_xyz)
    other = api.Context(0)
    foreign = api.Trajectory.from_points(other, xyz)
    dirs = T.fib_dirs(K, 1.0)
    axes = np.tile(np.float32([0, 0, 1]), (n, 1))
    f, fc = ctx.lib.wa_traj_tool_axes, ctx.lib.wa_traj_tool_check

    def tool_of(n_beads=3, dist16=16, r2=1):
        tl = api.torch_tool([dist16] * 3, [r2] * 3)
        tl.n_beads = n_beads
        return tl

    def with_row(a, i, row):
        a = np.array(a, np.float32)
        a[i] = row
        return a

    def call(g_=g.h, t_=t.h, dirs_=dirs, K_=K, tool=tool_of(), w=(1, 1, 1, 3, -1), want=None, off=(0, 10, n), n_legs=2, pf=None, pl=None,
             no=()):
        d, fe, lc = np.full(n, -7, np.int32), np.full(n * K, 77, np.uint8), np.full(2, -7, np.int64)
        s = L.ToolSummary()
        s.n = -9
        ww = L.ToolWeights(*w)
        off_ = np.asarray(off, np.int64)
        pf_, pl_ = (None if p is None else np.asarray(p, np.int32) for p in (pf, pl))
        want_ = None if want is None else np.ascontiguousarray(want, np.float32)
        dd = None if dirs_ is None else np.ascontiguousarray(dirs_, np.float32)
        rc = f(g_, t_, None if dd is None else dd.ctypes.data, K_, None if "tool" in no else C.byref(tool),
               None if "w" in no else C.byref(ww), None if want_ is None else want_.ctypes.data, None if "off" in no else off_.ctypes.data,
               n_legs, None if pf_ is None else pf_.ctypes.data, None if pl_ is None else pl_.ctypes.data, d.ctypes.data, fe.ctypes.data,
               lc.ctypes.data, None if "sum" in no else C.byref(s))
        return rc, (d == -7).all() and (fe == 77).all() and (lc == -7).all() and s.n == -9

    rc, untouched = call()
    assert rc == 0 and not untouched
    bad = [dict(g_=None), dict(t_=None), dict(dirs_=None), dict(no=("tool",)), dict(no=("w",)), dict(no=("off",)), dict(no=("sum",)),
           dict(t_=foreign.h), dict(K_=0), dict(K_=257), dict(K_=-1), dict(n_legs=-1),
           dict(tool=tool_of(0)), dict(tool=tool_of(65)), dict(tool=tool_of(dist16=-1)), dict(tool=tool_of(dist16=65537)),
           dict(tool=tool_of(r2=-1)), dict(tool=tool_of(r2=(1 << 30) + 1)),
           dict(w=(-1, 1, 1, 3, -1)), dict(w=(1025, 1, 1, 3, -1)), dict(w=(1, -1, 1, 3, -1)), dict(w=(1, 1025, 1, 3, -1)),
           dict(w=(1, 1, -1, 3, -1)), dict(w=(1, 1, 1025, 3, -1)), dict(w=(1, 1, 1, (1 << 30) + 1, -1)),
           dict(off=(1, 10, n)), dict(off=(0, 10, n - 1)), dict(off=(0, 10, n + 1)), dict(off=(0, n + 1, n)), dict(off=(0, -1, n)),
           dict(pf=(0, K)), dict(pf=(-2, 0)), dict(pl=(K, 0)), dict(pl=(0, -2)),
           dict(dirs_=with_row(dirs, 3, [0, 0, 0])), dict(dirs_=with_row(dirs, 3, [np.nan, 0, 1])), dict(dirs_=with_row(dirs, 0, [np.inf, 0, 1])),
           dict(want=with_row(np.zeros((n, 3)), 5, [np.nan, 0, 0])), dict(want=with_row(np.ones((n, 3)), n - 1, [0, -np.inf, 0])),
           dict(t_=nan.h), dict(t_=inf.h)]
    for kw in bad:
        rc, untouched = call(**kw)
        assert rc == ARG and untouched, kw
        if kw.get("g_", 1) is not None:
            assert b"wa_traj_tool_axes" in ctx.lib.wa_last_error(ctx.h), kw
    # optional outputs may be NULL
    s = L.ToolSummary()
    w = L.ToolWeights(1, 1, 1, 3, -1)
    off = np.array([0, n], np.int64)
    assert f(g.h, t.h, dirs.ctypes.data, K, C.byref(tool_of()), C.byref(w), None, off.ctypes.data, 1, None, None, None, None, None, C.byref(s)) == 0
    assert s.n == n

    # capacity: a leg above 2^22 samples (n * K above 2^33: test_capacity_of_samples_times_directions)
    big_n = (1 << 22) + 1
    big = api.Trajectory.from_points(ctx, np.zeros((big_n, 3), np.float32))
    d = np.full(4, -7, np.int32)
    s = L.ToolSummary()
    s.n = -9
    off = np.array([0, big_n], np.int64)
    assert f(g.h, big.h, dirs.ctypes.data, K, C.byref(tool_of()), C.byref(w), None, off.ctypes.data, 1, None, None, None, None, None,
             C.byref(s)) == CAPACITY and s.n == -9
    big.close()

    def check(g_=g.h, t_=t.h, axes_=axes, tool=tool_of(), near_add=3, no=()):
        b, nr = np.full(n, 77, np.uint8), np.full(n, 77, np.uint8)
        s = L.ToolSummary()
        s.n = -9
        a = None if axes_ is None else np.ascontiguousarray(axes_, np.float32)
        rc = fc(g_, t_, None if a is None else a.ctypes.data, None if "tool" in no else C.byref(tool), near_add, b.ctypes.data, nr.ctypes.data,
                None if "sum" in no else C.byref(s))
        return rc, (b == 77).all() and (nr == 77).all() and s.n == -9

    rc, untouched = check()
    assert rc == 0 and not untouched
    for kw in [dict(g_=None), dict(t_=None), dict(axes_=None), dict(no=("tool",)), dict(no=("sum",)), dict(t_=foreign.h), dict(tool=tool_of(0)),
               dict(tool=tool_of(dist16=65537)), dict(tool=tool_of(r2=-1)), dict(near_add=(1 << 30) + 1),
               dict(axes_=with_row(axes, 9, [0, 0, 0])), dict(axes_=with_row(axes, n - 1, [0, np.nan, 1])), dict(t_=nan.h), dict(t_=inf.h)]:
        rc, untouched = check(**kw)
        assert rc == ARG and untouched, kw
    s = L.ToolSummary()
    assert fc(g.h, t.h, axes.ctypes.data, C.byref(tool_of()), 3, None, None, C.byref(s)) == 0 and s.n == n
    for x in (t, nan, inf, foreign):
        x.close()
    other.close()


def test_capacity_of_samples_times_directions():
    """rule 9's second capacity case: K = 256 and n = 2^25 + 1 samples (n * K = 2^33 + 256, one sample above the limit) in legs that are
    all within 2^22 -- so the long-leg check cannot be what answers -- are refused with WA_ERR_CAPACITY and nothing is written.  (The
    other side of the boundary, n = 2^25 planned in full, maps 16 GiB and is not part of the suite.)"""
    K, n = 256, 1 << 25
    ctx = api.Context(0)                                   # its own: the 400 MB of samples go back when it closes
    empty = T.make_grid(np.ones((8, 8, 8), np.uint8), (8, 8, 8))
    g = grid_of(ctx, empty)
    dirs = T.fib_dirs(K, 1.2)
    tool, w = api.torch_tool([16], [1]), L.ToolWeights(1, 0, 1, 3, -1)
    pts = np.full((n + 1, 3), 3, np.float32)
    f = ctx.lib.wa_traj_tool_axes

    # 9 legs, eight of 2^22 and one of a single sample
    t = api.Trajectory.from_points(ctx, pts)
    del pts
    off = np.append(np.arange(9, dtype=np.int64) << 22, n + 1)
    d, lc = np.full(n + 1, -7, np.int32), np.full(9, -7, np.int64)
    s = L.ToolSummary()
    s.n = -9
    rc = f(g.h, t.h, dirs.ctypes.data, K, C.byref(tool), C.byref(w), None, off.ctypes.data, 9, None, None, d.ctypes.data, None, lc.ctypes.data,
           C.byref(s))
    assert rc == CAPACITY and (d == -7).all() and (lc == -7).all() and s.n == -9
    assert b"wa_traj_tool_axes" in ctx.lib.wa_last_error(ctx.h)
    t.close()
    g.close()
    ctx.close()


def test_stretched_and_shuffled_axis_tables(ctx):
    """every other grid here has unit axes; this one has a stretched x table (binary search over uneven spacing), a shuffled y table
    (the scan) and a repeated last z node, with samples on nodes, between them and outside"""
    rs = np.random.RandomState(21)
    nx, ny, nz = 23, 17, 11
    free = (rs.uniform(size=nx * ny * nz) >= 0.03).astype(np.uint8)
    cx = (np.cumsum(rs.uniform(0.05, 0.6, nx)) - 1).astype(np.float32)
    cy = rs.permutation(np.arange(ny)).astype(np.float32) * np.float32(0.5)
    cz = np.concatenate([np.arange(nz - 1), [nz - 2]]).astype(np.float32)
    grid = T.make_grid(free, (nx, ny, nz), (cx, cy, cz))
    xyz = np.stack([rs.uniform(-1.5, cx[-1] + 0.5, 150), rs.uniform(-1, 9, 150), rs.uniform(-1, 11, 150)], 1).astype(np.float32)
    xyz[::7] = np.stack([cx[rs.randint(0, nx, len(xyz[::7]))], cy[rs.randint(0, ny, len(xyz[::7]))], cz[rs.randint(0, nz, len(xyz[::7]))]], 1)
    want = rs.normal(size=(150, 3)).astype(np.float32)
    r = _same(ctx, grid, xyz, T.fib_dirs(65, 2.0), T.rod(5, 16 * 4, 1), T.weights(2, 1, 3, 4), want, [0, 40, 150])
    assert r["summary"]["n_outside"] > 0 and 0 < r["summary"]["n_blocked_pairs"] < 150 * 65


# ------------------------------------------------------------------ end to end: plan, stitch, fit, torch axes
def overhang_scene():
    """48^3, unit axes: a work piece (the floor slab z in 0..3) under an overhang (the slab z in 28..30 over x, y in 8..39); six weld
    points at z = 6 .. 9 under and beside the overhang.  A torch of 24 voxels standing upright reaches z = 30 .. 33 from there: under
    the overhang it hits it; leaning by up to 1.35 rad it stays below."""
    free = np.ones((48, 48, 48), np.uint8)                 # [z, y, x]
    free[0:4] = 0
    free[28:31, 8:40, 8:40] = 0
    pts = np.float32([[3, 4, 7], [14, 12, 6], [30, 16, 9], [36, 33, 7], [20, 36, 8], [4, 42, 6]])
    return T.make_grid(free, (48, 48, 48)), pts


def test_end_to_end_overhang(ctx):
    grid, pts = overhang_scene()
    g = grid_of(ctx, grid)
    ids = g.resolve(pts)
    hops, paths = api.geodesic_paths(g, ids[:-1], ids[1:])
    assert (hops > 0).all()
    poly = api.Trajectory.stitch(g, paths)
    _, samples, _, fs = poly.fit(g, degree=3, spacing=1.0, max_level=6, n_samples=601)
    assert fs["final"]["n_hit"] == 0
    xyz = samples.points()
    tool = T.rod(24, 16 * 24, 2)
    dirs = api.torch_cone(64, 1.35)
    assert np.array_equal(dirs, T.fib_dirs(64, 1.35))
    w = T.weights(1, 1, 1, 6, -1)
    up = np.tile(np.float32([0, 0, 1]), (len(xyz), 1))                                         # the wish: upright wherever that is possible
    o = samples.torch_axes(g, dirs, tool, want=up, **w)
    r = T.plan(grid, xyz, dirs, tool, w, want=up)
    assert np.array_equal(o["dir"], r["dir"]) and np.array_equal(o["feas"], r["feas"]) and o["summary"] == r["summary"]
    b, _, s = samples.torch_check(g, up, tool, 6)
    cb, _, cs = T.check(grid, xyz, up, tool, 6)
    assert np.array_equal(b, cb) and s == cs
    print("[torch] overhang 48^3 / 6 points, 601 samples: upright axis blocked at %d samples, planned axes at %d (%d directions used, "
          "%d blocked pairs of %d)" % (s["n_chosen_blocked"], o["summary"]["n_chosen_blocked"], len(set(o["dir"])),
                                      o["summary"]["n_blocked_pairs"], 601 * 64))
    assert o["summary"]["n_chosen_blocked"] == 0 and o["summary"]["n_no_dir"] == 0
    assert s["n_chosen_blocked"] > 0 and (o["dir"] == 0).sum() > 0 and len(set(o["dir"])) > 1   # upright where it can be, leaning under the overhang
    for x in (poly, samples, g):
        x.close()
