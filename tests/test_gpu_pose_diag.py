"""GPU tests of the diagonal pose paths (wa_grid_pose_diag_fields, _matrix, _paths; Grid.pose_diag_fields / pose_diag_matrix /
pose_diag_paths) against tests/pose_diag_ref.py, the header's definition in numpy, byte for byte.  tests/test_pose_diag_rules.py checks
the restatement itself.

Sizes: k_posed_level gives a wavefront 64 consecutive x of one row and a workgroup four rows (70 x 9 x 7: a tail of 6 lanes, 63 rows, so
the diagonal gather crosses the lane 63 / 64 seam and meets the grid's faces in every direction); a state word holds 64 directions
(K = 1, 5, 16, 33, 64 and 130: W = 3 with 2 live bits in the last plane); the ring has R = 2 .. 47 slots, the tunnel goes round it more
than ten times; the driver reads its termination words every 32 launches."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chamfer_ref as CR
import pose_diag_ref as PD
import pose_ref as PR
import pose_shortcut_ref as PS
import pose_weighted_ref as PW
import reach_ref as RR
import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, CAPACITY = 1, 7
STEP = [3, 4, 5]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def both(step, bands, turn_costs, pen=None):
    """one cost description for the library and for the restatement"""
    return api.pose_diag_costs(step, bands, turn_costs, pen), PD.Costs(step, bands, turn_costs, pen)


def near_pen(grid, top=3):
    """a penalty array from the distance field: `top` next to the metal, 1 within two voxels, 0 elsewhere; 200 on the metal (ignored)"""
    free, d2 = np.asarray(grid[0]).ravel() != 0, np.asarray(grid[1]).ravel()
    return np.where(~free, 200, np.where(d2 <= 1, top, np.where(d2 <= 4, 1, 0))).astype(np.uint8)


def same_paths(got, want, what):
    gh, gi, gk = got
    wh, wi, wk = want
    assert gh.dtype == np.int32 and np.array_equal(gh, wh), (what, gh, wh)
    for p in range(len(wh)):
        if wh[p] < 0:
            assert gi[p] is None and gk[p] is None, (what, p)
        else:
            assert gi[p].dtype == np.int64 and gk[p].dtype == np.int32
            assert np.array_equal(gi[p], wi[p]), (what, p, gi[p], wi[p])
            assert np.array_equal(gk[p], wk[p]), (what, p, gk[p], wk[p])


def all_pairs(pts, pins):
    idx = [(i, j) for i in range(len(pts)) for j in range(len(pts))]
    return ([pts[i] for i, _ in idx], [pts[j] for _, j in idx], [pins[i] for i, _ in idx], [pins[j] for _, j in idx])


def digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def check_case(ctx, c, max_turn, ac, rc, what, n_fields=2, base=None):
    """fields with states from the first points, the matrix with and without pins, all pair paths with their pins; returns the scene
    and how many moves of each class the paths made"""
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], max_turn, rc, base)
    g = grid_of(ctx, c["grid"])
    a = (c["dirs"], c["tool"], max_turn, ac)
    pts, pins = c["points"], c["pins"]
    cost, state = g.pose_diag_fields(*a, pts[:n_fields], pins[:n_fields], states=True)
    for i in range(n_fields):
        ws, wc = sc.levels(pts[i], pins[i])
        assert np.array_equal(cost[i], wc), (what, i, np.flatnonzero(cost[i] != wc)[:5])
        assert np.array_equal(state[i], ws), (what, i, np.argwhere(state[i] != ws)[:5])
    assert np.array_equal(g.pose_diag_fields(*a, pts[:n_fields], pins[:n_fields]), cost)   # without states
    m = g.pose_diag_matrix(*a, pts, pins)
    assert np.array_equal(m, sc.matrix(pts, pins)), (what, m)
    m = g.pose_diag_matrix(*a, pts)
    assert np.array_equal(m, sc.matrix(pts)), (what, m)
    assert (m > 0).any()
    if rc.pen is None:
        assert np.array_equal(m, m.T)
    else:
        adj = m - sc.pen[pts][None, :].astype(np.int32)
        assert np.array_equal(np.where(m >= 0, adj, -1), np.where(m.T >= 0, adj.T, -1))
    s, e, ps, pe = all_pairs(pts, pins)
    got = g.pose_diag_paths(*a, s, e, ps, pe)
    same_paths(got, sc.paths(s, e, ps, pe), what)
    by_class = np.zeros(3, np.int64)
    for p in range(len(s)):
        if got[0][p] >= 0:
            sc.check_path(got[1][p], got[2][p], s[p], e[p], ps[p], pe[p], int(got[0][p]))
            by_class += sc.moves_by_class(got[1][p])
    assert np.array_equal(g.occupancy(), np.asarray(c["grid"][0]))   # g is not modified
    g.close()
    print(what, "K", sc.K, "R", sc.R, "weights", sc.weights, "deepest level", sc.max_level, "moves by class", by_class.tolist())
    return sc, by_class


@pytest.mark.parametrize("with_pen", [False, True], ids=["no_pen", "pen"])
def test_wide_rows_cross_a_wavefront(ctx, with_pen):
    c = PR.wide_case()
    K = len(c["dirs"])
    thr = [K, max(1, K // 2), max(1, K // 4)]
    pen = RR.penalties(c["grid"], c["dirs"], c["tool"], thr) if with_pen else None
    bands = PW.bands_for(c["dirs"], c["max_turn"], 3)
    ac, rc = both(STEP, bands, [0, 1, 3, 6], pen)
    sc, by_class = check_case(ctx, c, c["max_turn"], ac, rc, ("wide", with_pen), n_fields=3)
    assert len(sc.weights) == 4 and sc.R == 10 + sc.P and sc.max_level > 64 and (sc.P >= 2) == with_pen
    assert by_class[1] > 0 and by_class[2] > 0


@pytest.fixture(scope="module")
def pillar_scenes():
    out = {}
    for gap in (4, 6):
        p = PR.pillars(gap)
        out[gap] = (p, PR.Scene(p["grid"], p["dirs"], p["tool"], -1))
    return out


@pytest.mark.parametrize("max_turn", [150000, 80000])
@pytest.mark.parametrize("gap", [4, 6])
def test_pillars_three_planes(ctx, pillar_scenes, gap, max_turn):
    p, base = pillar_scenes[gap]
    ac, rc = both(STEP, [0, 20000, 80000], [0, 2, 4, 8])
    sc = PD.Scene(p["grid"], p["dirs"], p["tool"], max_turn, rc, base)
    assert sc.K == 130
    g = grid_of(ctx, p["grid"])
    a = (p["dirs"], p["tool"], max_turn, ac)
    s, e = p["start"], p["end"]
    cost, state = g.pose_diag_fields(*a, [s], states=True)
    ws, wc = sc.levels(s)
    assert np.array_equal(cost[0], wc) and np.array_equal(state[0], ws)
    far = int(np.argmax(wc))                                   # the dearest voxel the start reaches: a reachable pair in every case
    assert wc[far] > 0
    pts = [s, e, 0, far]
    m = g.pose_diag_matrix(*a, pts)
    assert np.array_equal(m, sc.matrix(pts)) and np.array_equal(m, m.T) and m[0, 3] == wc[far]
    starts, ends = [s, e, 0, s], [e, s, e, far]
    got = g.pose_diag_paths(*a, starts, ends)
    same_paths(got, sc.paths(starts, ends), ("pillars", gap, max_turn))
    sc.check_path(got[1][3], got[2][3], s, far, -1, -1, int(got[0][3]))
    if max_turn == 80000 and gap == 4:
        assert got[0][0] == -1 and got[1][0] is None and m[0, 1] == -1 and cost[0][e] == -1   # no sequence of directions: no path, no error
    else:
        assert got[0][0] > 0
        sc.check_path(got[1][0], got[2][0], s, e, -1, -1, int(got[0][0]))
    g.close()


def test_tunnel_many_trips_round_the_ring(ctx):
    c = PR.tunnel_case()
    bands = PW.bands_for(c["dirs"], c["max_turn"], 3)
    ac, rc = both([2, 3, 4], bands, [0, 1, 2, 3])
    sc, _ = check_case(ctx, c, c["max_turn"], ac, rc, "tunnel", n_fields=1)
    assert sc.R == 6 and sc.max_level > 64 and sc.max_level > 10 * sc.R


BOX_TURNS = (-1, 150000, -1, -1)   # max_turn per seed: wide enough for the 5 and 16 directions of these scenes to fill two bands


@pytest.mark.parametrize("seed", range(4))
def test_box_scenes_with_torch_penalties(ctx, seed):
    """the penalties come from Grid.torch_penalties: the ring slot a lane pulls from varies along the row"""
    c = PR.box_case(seed)
    max_turn = BOX_TURNS[seed]
    K = len(c["dirs"])
    g = grid_of(ctx, c["grid"])
    thr = [K, max(1, K // 2), max(1, K // 4)]
    pen = g.torch_penalties(c["dirs"], c["tool"], thr)
    g.close()
    assert np.array_equal(pen, RR.penalties(c["grid"], c["dirs"], c["tool"], thr)) and len(set(pen.tolist())) >= 3
    bands = PW.bands_upto(c["dirs"], max_turn, 2)
    ac, rc = both(STEP, bands, [0, 2, 5], pen)
    sc, by_class = check_case(ctx, c, max_turn, ac, rc, ("box", seed))
    assert sc.P >= 2 and len(sc.weights) == 3 and by_class[1] + by_class[2] > 0


@pytest.mark.parametrize("K", [64, 1])
def test_a_full_plane_and_a_single_direction(ctx, K):
    grid, dirs, tool = RR.box_scene(1, 24)
    dirs = T.fib_dirs(64, 1.4, (0.3, -0.2, 1.0)) if K == 64 else dirs[2:3]
    max_turn = 60000 if K == 64 else 0
    c = dict(grid=grid, dirs=dirs, tool=tool, points=PR.spread_points(grid, 3), pins=[0, -1, K - 1])
    bands = PW.bands_for(dirs, max_turn, 3) if K == 64 else [0]
    ac, rc = both(STEP, bands, [0, 2, 3, 5][:len(bands) + 1], near_pen(grid, 4))
    sc, _ = check_case(ctx, c, max_turn, ac, rc, ("K", K))
    assert sc.K == K


def test_identity_1_steps_h_2h_3h_give_the_bytes_of_the_weighted_calls(ctx):
    """no pen: everything equals Grid.pose_weighted_* with hop_cost h on the device, and with h = 1 and zero turn costs Grid.pose_*"""
    for c, max_turn in ((PR.wide_case(), 30000), (PR.box_case(2), -1)):
        g = grid_of(ctx, c["grid"])
        pts, pins = c["points"], c["pins"]
        s, e, ps, pe = all_pairs(pts, pins)
        a = (c["dirs"], c["tool"], max_turn)
        bands, tc = PW.bands_for(c["dirs"], max_turn, 2), [0, 1, 4]
        for h in (1, 2, 3, 4, 5):
            w = api.pose_costs(h, bands, tc)
            d = api.pose_diag_costs([h, 2 * h, 3 * h], bands, tc)
            want_f = g.pose_weighted_fields(*a, w, pts[:2], pins[:2], states=True)
            got_f = g.pose_diag_fields(*a, d, pts[:2], pins[:2], states=True)
            assert np.array_equal(got_f[0], want_f[0]) and np.array_equal(got_f[1], want_f[1]) and (want_f[0] > 0).any()
            assert np.array_equal(g.pose_diag_matrix(*a, d, pts, pins), g.pose_weighted_matrix(*a, w, pts, pins))
            assert np.array_equal(g.pose_diag_matrix(*a, d, pts), g.pose_weighted_matrix(*a, w, pts))
            same_paths(g.pose_diag_paths(*a, d, s, e, ps, pe), g.pose_weighted_paths(*a, w, s, e, ps, pe), ("h", h))
        d = api.pose_diag_costs([1, 2, 3], [5000, 90000], [0, 0, 0])
        want_f = g.pose_fields(*a, pts[:2], pins[:2], states=True)
        got_f = g.pose_diag_fields(*a, d, pts[:2], pins[:2], states=True)
        assert np.array_equal(got_f[0], want_f[0]) and np.array_equal(got_f[1], want_f[1])
        assert np.array_equal(g.pose_diag_matrix(*a, d, pts, pins), g.pose_matrix(*a, pts, pins))
        same_paths(g.pose_diag_paths(*a, d, s, e, ps, pe), g.pose_paths(*a, s, e, ps, pe), "pose_*")
        g.close()


def test_identity_2_one_direction_is_the_chamfer_on_the_fit_grid(ctx):
    grid, dirs, tool = RR.box_scene(0, 24)
    dirs = dirs[2:3]
    pen = near_pen(grid, 5)
    g = grid_of(ctx, grid)
    fit = g.torch_fit(dirs, tool, min_dirs=1)
    free = fit.occupancy() != 0
    assert free.sum() < (np.asarray(grid[0]).ravel() != 0).sum()
    ff = np.flatnonzero(free)
    pts = [int(ff[i]) for i in np.linspace(0, len(ff) - 1, 5).astype(np.int64)]
    s, e = [pts[0]] * 4 + [pts[4]], pts[1:] + [pts[2]]
    wd, wl, wp = api.chamfer_weighted_paths(fit, STEP, pen, s, e)
    d = api.pose_diag_costs(STEP, [], [0], pen)
    gd, gi, gk = g.pose_diag_paths(dirs, tool, 0, d, s, e)
    assert np.array_equal(gd, wd) and (wd > 0).all()
    for p in range(len(s)):
        assert np.array_equal(gi[p], wp[p]) and len(gi[p]) == wl[p] and not gk[p].any()
    assert np.array_equal(g.pose_diag_fields(dirs, tool, 0, d, pts[:2]), fit.chamfer_weighted_fields(STEP, pen, pts[:2]))
    assert np.array_equal(g.pose_diag_matrix(dirs, tool, 0, d, pts), fit.chamfer_weighted_matrix(STEP, pen, pts))
    fit.close()
    g.close()


def test_identity_3_no_turn_gives_one_chamfer_field_per_direction(ctx):
    c = PR.box_case(0)
    K = len(c["dirs"])
    assert K == 5 and len({tuple(r) for r in T.quantise_all(c["dirs"]).tolist()}) == K
    opened = RR.open_dirs(c["grid"], c["dirs"], c["tool"])
    pen = near_pen(c["grid"])
    g = grid_of(ctx, c["grid"])
    src = c["points"][2]
    _, state = g.pose_diag_fields(c["dirs"], c["tool"], 0, api.pose_diag_costs(STEP, [], [0], pen), [src], states=True)
    _, _, _, axes = c["grid"]
    live = 0
    for k in range(K):
        if not opened[src, k]:
            assert (state[0, k] == -1).all()
            continue
        gk = api.Grid.from_occupancy(ctx, opened[:, k].astype(np.uint8), axes[0], axes[1], axes[2], 1.0, 0)
        assert np.array_equal(state[0, k], gk.chamfer_weighted_fields(STEP, pen, [src])[0]), k
        gk.close()
        live += 1
    assert live >= 1
    g.close()


def test_the_largest_ring(ctx):
    """step {16, 16, 16}, turn costs up to 15, penalties up to 15: R = 47"""
    grid, dirs, tool = RR.box_scene(3, 12)
    max_turn = 120000
    c = dict(grid=grid, dirs=dirs, tool=tool, points=PR.spread_points(grid, 4), pins=[-1, 3, -1, 0])
    free, d2 = np.asarray(grid[0]).ravel() != 0, np.asarray(grid[1]).ravel()
    pen = np.where(~free, 255, np.where(d2 <= 1, 15, np.where(d2 <= 9, 6, 0))).astype(np.uint8)
    ac, rc = both([16, 16, 16], PW.bands_for(dirs, max_turn, 4), [0, 3, 7, 11, 15], pen)
    sc, _ = check_case(ctx, c, max_turn, ac, rc, "R = 47")
    assert sc.R == 47 and len(sc.weights) == 5


def test_the_smallest_ring_is_the_chebyshev_distance(ctx):
    """step {1, 1, 1} on a grid without obstacles with one direction: R = 2 and cost = max(|dx|, |dy|, |dz|)"""
    nx, ny, nz = 70, 6, 5
    grid = T.make_grid(np.ones((nz, ny, nx), np.uint8), (nx, ny, nz))
    dirs, tool = T.fib_dirs(1, 0.1, (0.0, 0.0, 1.0)), T.rod(2, 16, 0)
    assert RR.open_dirs(grid, dirs, tool).all()
    srcs = [0, nx * ny * nz - 1, (2 * ny + 3) * nx + 64]
    g = grid_of(ctx, grid)
    ac, rc = both([1, 1, 1], [], [0])
    cost = g.pose_diag_fields(dirs, tool, -1, ac, srcs)
    for i, s in enumerate(srcs):
        assert np.array_equal(cost[i], CR.closed_form((1, 1, 1), (nx, ny, nz), s)), i
    sc = PD.Scene(grid, dirs, tool, -1, rc)
    assert sc.R == 2
    same_paths(g.pose_diag_paths(dirs, tool, -1, ac, srcs, srcs[::-1]), sc.paths(srcs, srcs[::-1]), "R = 2")
    g.close()


def test_pairs_sharing_a_start_with_different_pins(ctx):
    c = PR.wide_case()
    ac, rc = both(STEP, PW.bands_for(c["dirs"], c["max_turn"], 2), [0, 2, 5], near_pen(c["grid"]))
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], rc)
    g = grid_of(ctx, c["grid"])
    a, b, d = c["points"][0], c["points"][1], c["points"][4]
    open_a = np.flatnonzero(sc.opened[a])
    starts, ends = [a, a, a, a, b, a], [b, b, d, b, a, d]
    ps = [int(open_a[0]), int(open_a[-1]), int(open_a[0]), -1, -1, int(open_a[-1])]
    want = sc.paths(starts, ends, ps, None)
    assert (want[0] > 0).all() and len({tuple(w.tolist()) for w in want[2][:2]}) == 2   # the two pins give two different direction sequences
    same_paths(g.pose_diag_paths(c["dirs"], c["tool"], c["max_turn"], ac, starts, ends, ps), want, "shared starts")
    g.close()


def chunk_costs(c):
    return api.pose_diag_costs(STEP, PW.bands_for(c["dirs"], c["max_turn"], 3), [0, 1, 3, 6], near_pen(c["grid"]))


def test_chunking_does_not_change_the_bytes(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a child process) and all in one launch"""
    c = PR.wide_case()
    g = grid_of(ctx, c["grid"])
    a = (c["dirs"], c["tool"], c["max_turn"], chunk_costs(c))
    cost, state = g.pose_diag_fields(*a, c["points"], c["pins"], states=True)
    m = g.pose_diag_matrix(*a, c["points"], c["pins"])
    s, e, ps, pe = all_pairs(c["points"], c["pins"])
    ph, pi, pk = g.pose_diag_paths(*a, s, e, ps, pe)
    g.close()
    assert (ph > 0).any()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "import numpy as np\n"
             "import pose_ref as PR\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_pose_diag import grid_of, all_pairs, digest, chunk_costs\n"
             "c = PR.wide_case(); x = api.Context(0); g = grid_of(x, c['grid'])\n"
             "a = (c['dirs'], c['tool'], c['max_turn'], chunk_costs(c))\n"
             "cost, state = g.pose_diag_fields(*a, c['points'], c['pins'], states=True)\n"
             "s, e, ps, pe = all_pairs(c['points'], c['pins'])\n"
             "ph, pi, pk = g.pose_diag_paths(*a, s, e, ps, pe)\n"
             "print('digest', digest(cost, state), digest(g.pose_diag_matrix(*a, c['points'], c['pins'])), digest(ph, *[p for p in pi + pk if p is not None]))\n"
             % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    assert line[1:] == [digest(cost, state), digest(m), digest(ph, *[p for p in pi + pk if p is not None])]


def raw_paths(g, dirs, tool, max_turn, costs, starts, ends, off, fill=-7):
    """one raw wa_grid_pose_diag_paths call on prefilled outputs: (rc, ids, dirs, cost, lens)"""
    dirs = np.ascontiguousarray(dirs, np.float32)
    tool = api.torch_tool(*tool)
    starts, ends, off = (np.ascontiguousarray(a, np.int64) for a in (starts, ends, off))
    ids = np.full(max(int(off[-1]), 1), fill, np.int64)
    ks = np.full(max(int(off[-1]), 1), fill, np.int32)
    cost, lens = np.full(len(starts), fill, np.int32), np.full(len(starts), fill, np.int32)
    rc = g.ctx.lib.wa_grid_pose_diag_paths(g.h, dirs.ctypes.data, len(dirs), C.byref(tool), max_turn, C.byref(costs.c), starts.ctypes.data,
                                           ends.ctypes.data, None, None, len(starts), off.ctypes.data, ids.ctypes.data, ks.ctypes.data,
                                           cost.ctypes.data, lens.ctypes.data)
    return rc, ids, ks, cost, lens


def test_a_short_range_reports_capacity_after_all_counts(ctx):
    c = PR.box_case(0)
    ac, rc_ = both(STEP, PW.bands_for(c["dirs"], -1, 2), [0, 2, 5], near_pen(c["grid"]))
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], -1, rc_)
    g = grid_of(ctx, c["grid"])
    pts = c["points"]
    starts, ends = [pts[1], pts[3], pts[1], pts[5]], [pts[3], pts[5], pts[5], pts[1]]
    wd, wi, wk = sc.paths(starts, ends)
    assert (wd > 0).all()
    lens = np.array([len(p) for p in wi], np.int64)
    assert (lens != wd.astype(np.int64) + 1).all()          # the node count is not the cost + 1
    room = lens.copy()
    room[0] += 3          # a longer range than needed: its tail stays as it was
    room[2] -= 1          # one id short
    off = np.concatenate([[0], np.cumsum(room)])
    rc, ids, ks, cost, ln = raw_paths(g, c["dirs"], c["tool"], -1, ac, starts, ends, off)
    assert rc == CAPACITY
    assert np.array_equal(cost, wd) and np.array_equal(ln, lens)          # every pair's counts are delivered
    for p in (0, 1, 3):
        assert np.array_equal(ids[off[p]:off[p] + lens[p]], wi[p]) and np.array_equal(ks[off[p]:off[p] + lens[p]], wk[p])
    assert (ids[off[0] + lens[0]:off[1]] == -7).all() and (ks[off[0] + lens[0]:off[1]] == -7).all()
    assert (ids[off[2]:off[3]] == -7).all() and (ks[off[2]:off[3]] == -7).all()
    g.close()


def test_bad_arguments_leave_the_outputs_alone(ctx):
    c = PR.box_case(1)
    g = grid_of(ctx, c["grid"])
    lib = ctx.lib
    dirs = np.ascontiguousarray(c["dirs"], np.float32)
    K = len(dirs)
    tool = api.torch_tool(*c["tool"])
    free = np.asarray(c["grid"][0]).ravel()
    ok = np.array(c["points"][:2], np.int64)
    metal = np.array([c["points"][0], int(np.flatnonzero(free == 0)[0])], np.int64)
    pin_ok, pin_bad = np.array([-1, 0], np.int32), np.array([-1, K], np.int32)
    off = np.array([0, 100, 200], np.int64)
    good = api.pose_diag_costs(STEP, [1000, 20000], [0, 1, 4], near_pen(c["grid"]))

    def raw(step, n_bands, bands, tcs, pen=None):
        """a description the helper would refuse or the library must refuse"""
        s = L.PoseDiagCosts()
        s.n_bands = n_bands
        for i, b in enumerate(step):
            s.step[i] = b
        for i, b in enumerate(bands):
            s.turn_band[i] = b
        for i, t in enumerate(tcs):
            s.turn_cost[i] = t
        if pen is not None:
            s.pen = pen.ctypes.data
        return api.PoseDiagCosts(s, pen)

    def three(dirs_p, K_, max_turn, costs, ids, pins, null_len=False):
        """the three entry points with these arguments: every one returns WA_ERR_ARG and writes nothing"""
        cp = C.byref(costs.c) if costs is not None else None
        out = np.full((2, g.n), -7, np.int32)
        assert lib.wa_grid_pose_diag_fields(g.h, dirs_p, K_, C.byref(tool), max_turn, cp, ids.ctypes.data, pins.ctypes.data, 2, out.ctypes.data, None) == ARG
        assert (out == -7).all()
        m = np.full((2, 2), -7, np.int32)
        assert lib.wa_grid_pose_diag_matrix(g.h, dirs_p, K_, C.byref(tool), max_turn, cp, ids.ctypes.data, pins.ctypes.data, 2, m.ctypes.data) == ARG
        assert (m == -7).all()
        o, ks, h, ln = np.full(200, -7, np.int64), np.full(200, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int32)
        assert lib.wa_grid_pose_diag_paths(g.h, dirs_p, K_, C.byref(tool), max_turn, cp, ok.ctypes.data, ids.ctypes.data, None, pins.ctypes.data, 2,
                                           off.ctypes.data, o.ctypes.data, ks.ctypes.data, h.ctypes.data, None if null_len else ln.ctypes.data) == ARG
        assert (o == -7).all() and (ks == -7).all() and (h == -7).all() and (ln == -7).all()

    d = dirs.ctypes.data
    # rule 23's
    three(d, K, -2, good, ok, pin_ok)
    three(d, K, 3 * (1 << 20) + 1, good, ok, pin_ok)
    three(d, K, 1000, good, ok, pin_bad)
    three(d, K, 1000, good, metal, pin_ok)
    three(d, K, 1000, good, np.array([c["points"][0], g.n], np.int64), pin_ok)
    three(d, 0, 1000, good, ok, pin_ok)
    three(None, K, 1000, good, ok, pin_ok)
    # a step of 0 or 17, in every place
    for i in range(3):
        for bad in (0, 17, -1):
            step = list(STEP)
            step[i] = bad
            three(d, K, 1000, raw(step, 0, [], [0]), ok, pin_ok)
    # rule 35's
    three(d, K, 1000, None, ok, pin_ok)
    for nb in (-1, 5):
        three(d, K, 1000, raw(STEP, nb, [1, 2, 3, 4], [0, 1, 2, 3, 4]), ok, pin_ok)
    three(d, K, 1000, raw(STEP, 2, [500, 500], [0, 1, 2]), ok, pin_ok)              # bands not strictly ascending
    three(d, K, 1000, raw(STEP, 2, [500, 400], [0, 1, 2]), ok, pin_ok)
    three(d, K, 1000, raw(STEP, 1, [-1], [0, 1]), ok, pin_ok)
    three(d, K, 1000, raw(STEP, 1, [3 * (1 << 20) + 1], [0, 1]), ok, pin_ok)
    three(d, K, 1000, raw(STEP, 2, [500, 900], [0, 3, 2]), ok, pin_ok)              # costs decreasing
    three(d, K, 1000, raw(STEP, 2, [500, 900], [1, 2, 3]), ok, pin_ok)              # turn_cost[0] != 0
    three(d, K, 1000, raw(STEP, 2, [500, 900], [0, 2, 16]), ok, pin_ok)
    three(d, K, 1000, raw(STEP, 1, [500], [0, -1]), ok, pin_ok)
    pen = near_pen(c["grid"])
    pen[int(np.flatnonzero(free)[7])] = 16                                        # a free voxel above WA_POSE_COST_MAX
    three(d, K, 1000, raw(STEP, 1, [500], [0, 1], pen), ok, pin_ok)
    # len_out is required by _paths
    o, ks, h = np.full(200, -7, np.int64), np.full(200, -7, np.int32), np.full(2, -7, np.int32)
    assert lib.wa_grid_pose_diag_paths(g.h, d, K, C.byref(tool), 1000, C.byref(good.c), ok.ctypes.data, ok.ctypes.data, None, None, 2, off.ctypes.data,
                                       o.ctypes.data, ks.ctypes.data, h.ctypes.data, None) == ARG
    assert (o == -7).all() and (ks == -7).all() and (h == -7).all()
    # entries behind n_bands are ignored, the largest values are accepted, and a byte above 15 on the metal is ignored
    edge = raw([16, 16, 16], 1, [3 * (1 << 20), -5, -5, -5], [0, 15, -9, -9, -9], near_pen(c["grid"], 15))
    assert g.pose_diag_matrix(c["dirs"], c["tool"], 3 * (1 << 20), edge, ok).shape == (2, 2)
    with pytest.raises(ValueError):
        api.pose_diag_costs(STEP, [1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        api.pose_diag_costs([3, 4], [], [0])
    g.close()


def test_two_calls_give_the_same_bytes(ctx):
    c = PR.box_case(2)
    g = grid_of(ctx, c["grid"])
    costs = api.pose_diag_costs(STEP, PW.bands_for(c["dirs"], -1, 2), [0, 1, 3], near_pen(c["grid"]))
    a = (c["dirs"], c["tool"], -1, costs)
    s, e, ps, pe = all_pairs(c["points"], c["pins"])
    one = [(digest(*g.pose_diag_fields(*a, c["points"], c["pins"], states=True)), digest(g.pose_diag_matrix(*a, c["points"], c["pins"])),
            digest(*[p for r in g.pose_diag_paths(*a, s, e, ps, pe)[1:] for p in r if p is not None])) for _ in range(2)]
    assert one[0] == one[1]
    assert (g.pose_diag_matrix(*a, c["points"], c["pins"]) > 0).any()
    g.close()


def test_the_paths_feed_the_pose_shortcut(ctx):
    c = PR.wide_case()
    ac, rc = both(STEP, [0, 20000, 80000], [0, 2, 4, 8])
    g = grid_of(ctx, c["grid"])
    pts, pins = c["points"], c["pins"]
    s, e, ps, pe = all_pairs(pts, pins)
    cost, ids, ks = g.pose_diag_paths(c["dirs"], c["tool"], c["max_turn"], ac, s, e, ps, pe)
    keep = [p for p in range(len(s)) if cost[p] > 0]
    assert len(keep) >= 10
    ids, ks = [ids[p] for p in keep], [ks[p] for p in keep]
    wps, wks, holds, lengths, summ = api.pose_shortcut_paths(g, c["dirs"], c["tool"], c["max_turn"], ids, ks, 128)
    sc = PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    ww, wh, wl, ws = sc.batch(ids, ks, 128)
    straightened = 0
    for p in range(len(ids)):
        assert np.array_equal(wps[p], ids[p][ww[p]]) and np.array_equal(wks[p], ks[p][ww[p]]) and np.array_equal(holds[p], wh[p][:-1])
        for a, b, hold in zip(ww[p][:-1], ww[p][1:], holds[p]):
            if b - a > 1:          # a straightened stretch: its hold is open in every voxel the segment touches
                assert hold >= 0 and sc.cover_open(ids[p][a], ids[p][b], hold), (p, a, b, hold)
                straightened += 1
    assert np.array_equal(lengths.view(np.uint64), wl.view(np.uint64)) and summ == ws
    assert summ["n_waypoints"] < summ["n_nodes"] and straightened > 0
    g.close()


def test_plan_batch_with_diagonal_pose_paths(ctx):
    """examples/plan_batch.py --pose-diagonal: the same pairs reached, and no longer paths than the staircase planner's"""
    base = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", "--torch", "64", "--pose-paths", "150000",
            "--shortcut", "--pose-shortcut"]
    outs = []
    for extra in ([], ["--pose-diagonal"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
        outs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    stairs, diag = outs
    assert "pose_diagonal" not in stairs
    pd = diag["pose_diagonal"]
    assert pd["step"] == STEP and diag["all_reached"] == stairs["all_reached"]
    assert diag["pose_paths"]["unreachable_pairs"] == stairs["pose_paths"]["unreachable_pairs"] and pd["pairs_reached"] > 0
    assert pd["length_total"] <= pd["staircase"]["length_total"]
    assert sum(pd["moves_by_class"][1:]) > 0
    print(json.dumps(pd))
