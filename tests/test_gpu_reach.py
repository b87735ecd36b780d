"""GPU tests of the torch-fit planning grids (wa_grid_tool_reach, wa_grid_tool_fit, wa_grid_tool_penalties; Grid.torch_reach / torch_fit /
torch_penalties) against tests/reach_ref.py, the header's definition in numpy, byte for byte.

Sizes: k_reach gives a wavefront 64 consecutive x of one row and a workgroup four rows, so nx sits on and around 64 (1, 63, 64, 65, 130)
with ny * nz = 45 rows (no multiple of 4, ny = 9 neither); a mask word holds 64 directions, so K sits on and around 64 and at both ends
(1, 63, 64, 65, 129, 256); beads are loaded four at a time (1, 24, 64 beads) and K * n_beads = 256 * 64 needs 128 KiB of LDS.  The
box scenes have far AND near free voxels, so both sides of the far-voxel shortcut are compared with a restatement that has none."""
import ctypes as C

import numpy as np
import pytest

import chamfer_weighted_ref as CW
import geodesic_ref as GR
import reach_ref as RR
import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG = 1


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def speckled(seed, dims, p=0.05):
    rs = np.random.RandomState(500 + seed)
    free = (rs.uniform(size=dims[::-1]) > p).astype(np.uint8)
    return T.make_grid(free, dims)


def _same(ctx, grid, dirs, tool, what=None):
    """one call against the restatement: masks, counts, summary; then the call without masks.  Returns the reference result."""
    rm, rc, rs = RR.reach(grid, dirs, tool)
    g = grid_of(ctx, grid)
    m, c, s = g.torch_reach(dirs, tool)
    assert m.shape == rm.shape and m.dtype == np.uint64 and c.dtype == np.uint16
    print(what, "summary", s, "reference", rs)
    assert np.array_equal(c, rc), (what, np.flatnonzero(c != rc)[:5], c[c != rc][:5], rc[c != rc][:5])
    assert np.array_equal(m, rm), (what, np.argwhere(m != rm)[:5])
    assert s == rs, (what, s, rs)
    m2, c2, s2 = g.torch_reach(dirs, tool, masks=False)
    assert m2 is None and np.array_equal(c2, rc) and s2 == rs, what
    g.close()
    return rm, rc, rs


# (nx, ny, nz), K, n_beads, rod length in sixteenths: not the product of the maxima -- the restatement is the slow side
SHAPES = [((1, 9, 5), 1, 1, 40), ((63, 9, 5), 63, 24, 150), ((64, 9, 5), 64, 1, 70), ((65, 9, 5), 65, 24, 200),
          ((130, 9, 5), 129, 1, 90), ((130, 9, 5), 64, 24, 120), ((65, 5, 3), 256, 64, 100), ((1, 1, 1), 3, 2, 16),
          ((64, 4, 1), 256, 1, 33)]


@pytest.mark.parametrize("dims,K,nb,length", SHAPES)
def test_masks_counts_summary_at_the_kernel_edges(ctx, dims, K, nb, length):
    rs = np.random.RandomState(K * 131 + nb)
    grid = speckled(K + nb, dims)
    dirs = rs.normal(size=(K, 3)).astype(np.float32)           # every side of the grid is left by some bead
    tool = (np.rint(np.linspace(0, length, nb)).astype(np.int64) if nb > 1 else np.array([length], np.int64), rs.randint(0, 4, nb).astype(np.int64))
    _, rc, s = _same(ctx, grid, dirs, tool, (dims, K, nb))
    if np.prod(dims) > 100:
        assert 0 < s["n_blocked_pairs"] < K * s["n_free"]        # the scene decides something


def test_long_beads_on_a_tiny_grid(ctx):
    grid = speckled(3, (5, 6, 7), 0.1)
    dirs = np.concatenate([np.eye(3), -np.eye(3), np.random.RandomState(5).normal(size=(11, 3))]).astype(np.float32)
    _same(ctx, grid, dirs, (np.array([0, 16, 23, 40000, 65536], np.int64), np.array([0, 1, 2, 1 << 30, 7], np.int64)), "long beads")


def test_obstacle_free_and_full_grids(ctx):
    dims = (70, 5, 3)
    n = int(np.prod(dims))
    dirs, tool = T.fib_dirs(70, 1.0), T.rod(5, 48, 2)
    _, c, s = _same(ctx, T.make_grid(np.ones(n, np.uint8), dims), dirs, tool, "free")
    assert (c == 70).all() and s == dict(n_free=n, n_no_dir=0, n_all_dirs=n, n_blocked_pairs=0)
    _, c, s = _same(ctx, T.make_grid(np.zeros(n, np.uint8), dims), dirs, tool, "full")
    assert (c == 0).all() and s == dict(n_free=0, n_no_dir=0, n_all_dirs=0, n_blocked_pairs=0)


@pytest.mark.parametrize("seed,m", [(0, 24), (1, 24), (2, 32), (3, 48)])
def test_box_scenes_with_far_and_near_voxels(ctx, seed, m):
    grid, dirs, tool = RR.box_scene(seed, m)
    far, near = RR.far_near(grid, tool)
    assert far.any() and near.any()
    _, rc, _ = _same(ctx, grid, dirs, tool, ("boxes", seed, m))
    assert (rc[far] == len(dirs)).all() and (rc[near] < len(dirs)).any()


def test_two_calls_give_the_same_bytes(ctx):
    grid, dirs, tool = RR.box_scene(4, 24)
    g = grid_of(ctx, grid)
    a, b = g.torch_reach(dirs, tool), g.torch_reach(dirs, tool)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    thr = [3, 1, 3]
    assert np.array_equal(g.torch_penalties(dirs, tool, thr), g.torch_penalties(dirs, tool, thr))
    f1, f2 = g.torch_fit(dirs, tool, 2), g.torch_fit(dirs, tool, 2)
    assert np.array_equal(f1.occupancy(), f2.occupancy()) and f1.n_free == f2.n_free
    assert np.array_equal(g.occupancy(), np.asarray(grid[0]))   # g is not modified
    for x in (f1, f2, g):
        x.close()


def test_masks_agree_with_the_trajectory_planner(ctx):
    """every voxel centre as a trajectory through wa_traj_tool_axes: its feasibility bytes say blocked exactly where the mask bit is clear"""
    grid = T.boxes_grid(np.random.RandomState(11), 12, 4)
    g = grid_of(ctx, grid)
    dirs, tool = T.fib_dirs(70, 2.0, (0.3, -0.2, 1.0)), T.rod(6, 16 * 5, 1)
    cx, cy, cz = g.coords()
    z, y, x = np.meshgrid(cz, cy, cx, indexing="ij")
    t = api.Trajectory.from_points(ctx, np.stack([x.ravel(), y.ravel(), z.ravel()], 1))
    ids = t.clearance(g)[0]
    assert np.array_equal(ids, np.arange(g.n))
    feas = t.torch_axes(g, dirs, tool)["feas"]
    mask, count, _ = g.torch_reach(dirs, tool)
    free = g.occupancy() != 0
    k = np.arange(len(dirs))
    bit = ((mask[k >> 6][:, ids] >> (k & 63).astype(np.uint64)[:, None]) & np.uint64(1)).T.astype(bool)     # [n, K]
    assert np.array_equal((feas == 255)[free], ~bit[free])
    assert not bit[~free].any() and 0 < bit[free].sum() < bit[free].size
    t.close()
    g.close()


@pytest.fixture(scope="module")
def boxes24(ctx):
    grid, dirs, tool = RR.box_scene(5, 24)
    g = grid_of(ctx, grid)
    count = RR.reach(grid, dirs, tool)[1]
    yield grid, dirs, tool, g, count
    g.close()


@pytest.mark.parametrize("min_dirs", [1, None])
@pytest.mark.parametrize("keep_r2", [0, 5])
def test_fit_equals_the_rule(ctx, boxes24, min_dirs, keep_r2):
    grid, dirs, tool, g, count = boxes24
    K = len(dirs)
    min_dirs = K if min_dirs is None else min_dirs
    free = np.asarray(grid[0]) != 0
    closed = np.flatnonzero(free & (count < min_dirs))
    assert len(closed), "the scene closes voxels"
    keep = closed[[0, len(closed) // 2, -1]]                   # bubbles around voxels the rule would close
    for ids in ([], keep):
        want = RR.fit(grid, dirs, tool, min_dirs, ids, keep_r2, count=count)
        f = g.torch_fit(dirs, tool, min_dirs, ids, keep_r2)
        assert np.array_equal(f.occupancy(), want) and f.n_free == int(want.sum()), (min_dirs, keep_r2, len(ids))
        assert f.reach_summary == RR.summarise(grid[0], count, K)
        assert (f.nx, f.ny, f.nz, f.precision, f.wall) == (g.nx, g.ny, g.nz, g.precision, g.wall)
        if len(ids):
            assert want[keep].all() and want.sum() > RR.fit(grid, dirs, tool, min_dirs, count=count).sum()
        f.close()


def test_fit_grid_plans(ctx, boxes24):
    grid, dirs, tool, g, count = boxes24
    want = RR.fit(grid, dirs, tool, 3, count=count)
    f = g.torch_fit(dirs, tool, 3)
    pts = np.flatnonzero(want)[[0, 77, 1500, -1]]
    assert np.array_equal(f.geodesic_matrix(pts), GR.matrix(want, grid[2], pts))
    f.close()


def test_fit_argument_errors_leave_out_alone(ctx, boxes24):
    grid, dirs, tool, g, _ = boxes24
    lib, K = ctx.lib, len(dirs)
    d = np.ascontiguousarray(dirs, np.float32)
    tb = api.torch_tool(*tool)
    occupied = int(np.flatnonzero(np.asarray(grid[0]) == 0)[0])
    free_id = int(np.flatnonzero(np.asarray(grid[0]) != 0)[0])
    SENT = 0x5a5a5a5a

    def call(dirs=d, K=K, tool=tb, min_dirs=1, keep=(free_id,), n_keep=None, keep_r2=0, out=True):
        h = C.c_void_p(SENT)
        keep = np.asarray(keep, np.int64)
        rc = lib.wa_grid_tool_fit(g.h, dirs.ctypes.data if dirs is not None else None, K, C.byref(tool) if tool is not None else None, min_dirs,
                                  keep.ctypes.data if len(keep) else None, len(keep) if n_keep is None else n_keep, keep_r2,
                                  C.byref(h) if out else None, None)
        assert h.value == SENT or rc == 0, "out was written by a refused call"
        if rc == 0:
            lib.wa_grid_destroy(h)
        return rc

    assert call() == 0
    bad_tool = [api.torch_tool(*tool) for _ in range(4)]
    bad_tool[0].n_beads = 0
    bad_tool[1].n_beads = 65
    bad_tool[2].dist16[0] = 65537
    bad_tool[3].r2[0] = -1
    nan, zero = d.copy(), d.copy()
    nan[K - 1, 1] = np.nan
    zero[0] = 0
    cases = dict(no_dirs=dict(dirs=None), no_tool=dict(tool=None), no_out=dict(out=False), K0=dict(K=0), K257=dict(K=257),
                 min0=dict(min_dirs=0), min_above_K=dict(min_dirs=K + 1), r2_negative=dict(keep_r2=-1), n_keep_negative=dict(n_keep=-1),
                 keep_outside=dict(keep=(g.n,)), keep_negative=dict(keep=(-1,)), keep_occupied=dict(keep=(free_id, occupied)),
                 nan=dict(dirs=nan), zero=dict(dirs=zero), **{"tool%d" % i: dict(tool=t) for i, t in enumerate(bad_tool)})
    for name, kw in cases.items():
        assert call(**kw) == ARG, name
    s = L.ReachSummary()
    cnt = np.zeros(g.n, np.uint16)
    assert lib.wa_grid_tool_reach(g.h, d.ctypes.data, K, C.byref(tb), None, cnt.ctypes.data, None) == ARG
    assert lib.wa_grid_tool_reach(g.h, nan.ctypes.data, K, C.byref(tb), None, cnt.ctypes.data, C.byref(s)) == ARG and not cnt.any()
    pen = np.full(g.n, 77, np.uint8)
    for thr in ([-1], [65536], list(range(32))):
        th = np.asarray(thr, np.int32)
        assert lib.wa_grid_tool_penalties(g.h, d.ctypes.data, K, C.byref(tb), th.ctypes.data, len(th), pen.ctypes.data) == ARG, thr
    assert lib.wa_grid_tool_penalties(g.h, d.ctypes.data, K, C.byref(tb), None, 1, pen.ctypes.data) == ARG
    assert lib.wa_grid_tool_penalties(g.h, d.ctypes.data, K, C.byref(tb), None, -1, pen.ctypes.data) == ARG
    assert (pen == 77).all()


def test_penalties_equal_the_rule_and_feed_the_weighted_search(ctx, boxes24):
    grid, dirs, tool, g, count = boxes24
    K = len(dirs)
    for thr in ([], [K], [K, 1, K // 2, 1, 0, 65535], list(range(1, 32))):
        assert np.array_equal(g.torch_penalties(dirs, tool, thr), RR.penalties(grid, dirs, tool, thr, count=count)), thr
    thr = [K, 1, K // 2, 1]
    pen = g.torch_penalties(dirs, tool, thr)
    assert pen.max() == 4 and pen.min() == 0
    free, dims = np.asarray(grid[0]), grid[2]
    ids = np.flatnonzero(free)
    starts, ends = [int(ids[0]), int(ids[-1])], [int(ids[-1]), int(ids[len(ids) // 2])]
    step = (2, 3, 4)
    dist, lens, paths = api.chamfer_weighted_paths(g, step, pen, starts, ends)
    rd, rl, rp = CW.paths(free, np.asarray(step), pen, dims, starts, ends)
    assert np.array_equal(dist, rd) and np.array_equal(lens, rl) and all(np.array_equal(a, b) for a, b in zip(paths, rp))


def test_tunnel_scene_end_to_end(ctx):
    """the planner runs through the tunnel, where the torch has no direction; on the fit grid it goes over the wall"""
    sc = RR.tunnel_scene()
    grid, dirs, tool = sc["grid"], sc["dirs"], sc["tool"]
    free, _, dims, _ = grid
    _, count, _ = RR.reach(grid, dirs, tool)
    ref_path = GR.walk_back(GR.field(free, dims, sc["start"]), dims, sc["end"])
    ref_fit = RR.fit(grid, dirs, tool, 1, count=count)
    ref_path2 = GR.walk_back(GR.field(ref_fit, dims, sc["start"]), dims, sc["end"])
    g = grid_of(ctx, grid)
    vox = RR.voxels(dims).astype(np.float32)                   # unit axes: a voxel's centre is its index triple

    def plan(on):
        hops, paths = api.geodesic_paths(on, [sc["start"]], [sc["end"]])
        t = api.Trajectory.from_points(ctx, vox[paths[0]])
        s = t.torch_axes(g, dirs, tool, feas=False)["summary"]
        t.close()
        return int(hops[0]), paths[0], s["n_no_dir"]

    hops, path, no_dir = plan(g)
    print("on g: hops", hops, "n_no_dir", no_dir)
    assert hops == len(ref_path) - 1 and np.array_equal(path, ref_path) and no_dir == int((count[ref_path] == 0).sum())
    f = g.torch_fit(dirs, tool, 1)
    assert np.array_equal(f.occupancy(), ref_fit)
    hops2, path2, no_dir2 = plan(f)
    print("on the fit grid: hops", hops2, "n_no_dir", no_dir2)
    assert hops2 == len(ref_path2) - 1 and np.array_equal(path2, ref_path2) and no_dir2 == int((count[ref_path2] == 0).sum()) == 0
    assert hops2 > hops and no_dir > 0
    f.close()
    g.close()
