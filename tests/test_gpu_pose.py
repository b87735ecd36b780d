"""GPU tests of the exact pose paths (wa_grid_pose_fields, wa_grid_pose_matrix, wa_grid_pose_paths; Grid.pose_fields / pose_matrix /
pose_paths) against tests/pose_ref.py, the header's definition in numpy, byte for byte.  tests/test_pose_rules.py checks the restatement
itself and that each scene used here decides something.

Sizes: k_pose_level gives a wavefront 64 consecutive x of one row and a workgroup four rows (70 x 9 x 7: a tail of 6 lanes, 63 rows);
a state word holds 64 directions (K = 5, 16, 32, 33 and 130: W = 3 with 2 live bits in the last plane); the driver reads its
termination words every 32 launches (34 levels on the pillars, more than 64 in the tunnel and the wide scene)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_ref as PR
import reach_ref as RR
import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, CAPACITY = 1, 7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


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


def check_case(ctx, c, what, n_fields=2):
    """fields with states from the first points, the matrix with and without pins, all pair paths with their pins"""
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    g = grid_of(ctx, c["grid"])
    pts, pins = c["points"], c["pins"]
    hops, state = g.pose_fields(c["dirs"], c["tool"], c["max_turn"], pts[:n_fields], pins[:n_fields], states=True)
    for i in range(n_fields):
        ws, wh = sc.levels(pts[i], pins[i])
        assert np.array_equal(hops[i], wh), (what, i, np.flatnonzero(hops[i] != wh)[:5])
        assert np.array_equal(state[i], ws), (what, i, np.argwhere(state[i] != ws)[:5])
    assert np.array_equal(g.pose_fields(c["dirs"], c["tool"], c["max_turn"], pts[:n_fields], pins[:n_fields]), hops)   # without states
    m = g.pose_matrix(c["dirs"], c["tool"], c["max_turn"], pts, pins)
    assert np.array_equal(m, sc.matrix(pts, pins)), (what, m)
    assert np.array_equal(m, m.T)
    m = g.pose_matrix(c["dirs"], c["tool"], c["max_turn"], pts)
    assert np.array_equal(m, sc.matrix(pts)) and np.array_equal(m, m.T), (what, m)
    s, e, ps, pe = all_pairs(pts, pins)
    same_paths(g.pose_paths(c["dirs"], c["tool"], c["max_turn"], s, e, ps, pe), sc.paths(s, e, ps, pe), what)
    assert np.array_equal(g.occupancy(), np.asarray(c["grid"][0]))   # g is not modified
    g.close()


@pytest.fixture(scope="module")
def pillars():
    p = PR.pillars(4)
    return p, PR.Scene(p["grid"], p["dirs"], p["tool"], -1)


@pytest.mark.parametrize("max_turn", [-1, 80000, 150000])
def test_pillars_fields_matrix_paths(ctx, pillars, max_turn):
    p, sc0 = pillars
    sc = sc0.with_turn(max_turn)
    g = grid_of(ctx, p["grid"])
    s, e = p["start"], p["end"]
    hops, state = g.pose_fields(p["dirs"], p["tool"], max_turn, [s], states=True)
    ws, wh = sc.levels(s)
    print("pillars", max_turn, "hops", hops[0][e], "deepest", state.max())
    assert np.array_equal(hops[0], wh) and np.array_equal(state[0], ws)
    assert hops[0][e] == {-1: 9, 80000: -1, 150000: 13}[max_turn]
    pts = [s, e, 0, int(np.prod(p["grid"][2])) - 1]
    m = g.pose_matrix(p["dirs"], p["tool"], max_turn, pts)
    assert np.array_equal(m, sc.matrix(pts)) and np.array_equal(m, m.T)
    same_paths(g.pose_paths(p["dirs"], p["tool"], max_turn, [s, e, 0], [e, s, e]), sc.paths([s, e, 0], [e, s, e]), ("pillars", max_turn))
    g.close()


def test_tunnel_more_than_64_levels(ctx):
    check_case(ctx, PR.tunnel_case(), "tunnel")


def test_wide_rows_cross_a_wavefront(ctx):
    check_case(ctx, PR.wide_case(), "wide", n_fields=3)


@pytest.mark.parametrize("seed", range(4))
def test_box_scenes(ctx, seed):
    check_case(ctx, PR.box_case(seed), ("box", seed))


def test_pins(ctx):
    c = PR.box_case(2)
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    g = grid_of(ctx, c["grid"])
    a, b = c["points"][1], c["points"][4]
    K = sc.K
    ka, kb = int(np.flatnonzero(sc.opened[a])[-1]), int(np.flatnonzero(sc.opened[b])[0])
    # a voxel next to a box with a closed direction, reached from a: the pin on the closed direction gives -1 everywhere, no error
    shut = np.argwhere(sc.free[:, None] & ~sc.opened & sc.opened.any(1)[:, None])
    v, kc = int(shut[0][0]), int(shut[0][1])
    starts, ends = [a, a, a, v, a, a], [b, b, v, b, a, a]
    ps, pe = [ka, -1, -1, kc, -1, ka], [-1, kb, kc, -1, -1, ka]
    want = sc.paths(starts, ends, ps, pe)
    assert want[0][0] > 0 and want[0][1] > 0 and want[0][2] == -1 and want[0][3] == -1 and want[0][4] == 0 and want[0][5] == 0
    got = g.pose_paths(c["dirs"], c["tool"], c["max_turn"], starts, ends, ps, pe)
    same_paths(got, want, "pins")
    assert got[2][0][0] == ka and got[2][1][-1] == kb and len(got[1][4]) == 1
    hops, state = g.pose_fields(c["dirs"], c["tool"], c["max_turn"], [v], [kc], states=True)
    assert (hops == -1).all() and (state == -1).all()
    m = g.pose_matrix(c["dirs"], c["tool"], c["max_turn"], [v, a], [kc, -1])
    assert m.tolist() == [[-1, -1], [-1, 0]]
    assert K > 1
    g.close()


def test_pairs_sharing_a_start_with_different_pins(ctx):
    c = PR.wide_case()
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    g = grid_of(ctx, c["grid"])
    a, b, d = c["points"][0], c["points"][1], c["points"][4]
    open_a = np.flatnonzero(sc.opened[a])
    starts, ends = [a, a, a, a, b, a], [b, b, d, b, a, d]
    ps = [int(open_a[0]), int(open_a[-1]), int(open_a[0]), -1, -1, int(open_a[-1])]
    want = sc.paths(starts, ends, ps, None)
    assert len({tuple(w.tolist()) for w in want[2][:2]}) == 2          # the two pins give two different direction sequences
    same_paths(g.pose_paths(c["dirs"], c["tool"], c["max_turn"], starts, ends, ps), want, "shared starts")
    g.close()


def test_chunking_does_not_change_the_bytes(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a child process) and all in one launch"""
    c = PR.wide_case()
    g = grid_of(ctx, c["grid"])
    hops, state = g.pose_fields(c["dirs"], c["tool"], c["max_turn"], c["points"], c["pins"], states=True)
    m = g.pose_matrix(c["dirs"], c["tool"], c["max_turn"], c["points"], c["pins"])
    s, e, ps, pe = all_pairs(c["points"], c["pins"])
    ph, pi, pk = g.pose_paths(c["dirs"], c["tool"], c["max_turn"], s, e, ps, pe)
    g.close()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "import numpy as np, hashlib\n"
             "import pose_ref as PR\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_pose import grid_of, all_pairs, digest\n"
             "c = PR.wide_case(); x = api.Context(0); g = grid_of(x, c['grid'])\n"
             "a = (c['dirs'], c['tool'], c['max_turn'])\n"
             "hops, state = g.pose_fields(*a, c['points'], c['pins'], states=True)\n"
             "s, e, ps, pe = all_pairs(c['points'], c['pins'])\n"
             "ph, pi, pk = g.pose_paths(*a, s, e, ps, pe)\n"
             "print('digest', digest(hops, state), digest(g.pose_matrix(*a, c['points'], c['pins'])), digest(ph, *[p for p in pi + pk if p is not None]))\n"
             % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    assert line[1:] == [digest(hops, state), digest(m), digest(ph, *[p for p in pi + pk if p is not None])]


def digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def raw_paths(g, dirs, tool, max_turn, starts, ends, off, fill=-7):
    """one raw wa_grid_pose_paths call on prefilled outputs: (rc, ids, dirs, hops, lens)"""
    dirs = np.ascontiguousarray(dirs, np.float32)
    tool = api.torch_tool(*tool)
    starts, ends, off = (np.ascontiguousarray(a, np.int64) for a in (starts, ends, off))
    ids = np.full(max(int(off[-1]), 1), fill, np.int64)
    ks = np.full(max(int(off[-1]), 1), fill, np.int32)
    hops, lens = np.full(len(starts), fill, np.int32), np.full(len(starts), fill, np.int32)
    rc = g.ctx.lib.wa_grid_pose_paths(g.h, dirs.ctypes.data, len(dirs), C.byref(tool), max_turn, starts.ctypes.data, ends.ctypes.data, None, None,
                                      len(starts), off.ctypes.data, ids.ctypes.data, ks.ctypes.data, hops.ctypes.data, lens.ctypes.data)
    return rc, ids, ks, hops, lens


def test_a_short_range_reports_capacity_after_all_counts(ctx):
    c = PR.box_case(0)
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    g = grid_of(ctx, c["grid"])
    pts = c["points"]
    starts, ends = [pts[1], pts[3], pts[1], pts[5]], [pts[3], pts[5], pts[5], pts[1]]
    wh, wi, wk = sc.paths(starts, ends)
    assert (wh > 0).all()
    lens = wh.astype(np.int64) + 1
    room = lens.copy()
    room[0] += 3          # a longer range than needed: its tail stays as it was
    room[2] -= 1          # one id short
    off = np.concatenate([[0], np.cumsum(room)])
    rc, ids, ks, hops, ln = raw_paths(g, c["dirs"], c["tool"], c["max_turn"], starts, ends, off)
    assert rc == CAPACITY
    assert np.array_equal(hops, wh) and np.array_equal(ln, lens)          # every pair's counts are delivered
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

    def three(dirs_p, K_, max_turn, ids, pins):
        """the three entry points with these arguments: every one returns WA_ERR_ARG and writes nothing"""
        hops = np.full((2, g.n), -7, np.int32)
        assert lib.wa_grid_pose_fields(g.h, dirs_p, K_, C.byref(tool), max_turn, ids.ctypes.data, pins.ctypes.data, 2, hops.ctypes.data, None) == ARG
        assert (hops == -7).all()
        m = np.full((2, 2), -7, np.int32)
        assert lib.wa_grid_pose_matrix(g.h, dirs_p, K_, C.byref(tool), max_turn, ids.ctypes.data, pins.ctypes.data, 2, m.ctypes.data) == ARG
        assert (m == -7).all()
        out, ks, h, ln = np.full(200, -7, np.int64), np.full(200, -7, np.int32), np.full(2, -7, np.int32), np.full(2, -7, np.int32)
        assert lib.wa_grid_pose_paths(g.h, dirs_p, K_, C.byref(tool), max_turn, ok.ctypes.data, ids.ctypes.data, None, pins.ctypes.data, 2,
                                      off.ctypes.data, out.ctypes.data, ks.ctypes.data, h.ctypes.data, ln.ctypes.data) == ARG
        assert (out == -7).all() and (ks == -7).all() and (h == -7).all() and (ln == -7).all()

    three(dirs.ctypes.data, K, -2, ok, pin_ok)
    three(dirs.ctypes.data, K, 3 * (1 << 20) + 1, ok, pin_ok)
    three(dirs.ctypes.data, K, 1000, ok, pin_bad)
    three(dirs.ctypes.data, K, 1000, metal, pin_ok)
    three(dirs.ctypes.data, K, 1000, np.array([c["points"][0], g.n], np.int64), pin_ok)
    three(dirs.ctypes.data, 0, 1000, ok, pin_ok)
    three(None, K, 1000, ok, pin_ok)
    # the largest max_turn is accepted
    assert g.pose_matrix(c["dirs"], c["tool"], 3 * (1 << 20), ok).shape == (2, 2)
    g.close()


@pytest.mark.parametrize("which", ["no_limit", "one_direction", "no_obstacles"])
def test_reductions_on_the_device(ctx, which):
    """against Grid.geodesic_matrix of Grid.torch_fit(min_dirs=1), everything on the device"""
    if which == "no_obstacles":
        dims = (70, 5, 3)
        grid = T.make_grid(np.ones(int(np.prod(dims)), np.uint8), dims)
        dirs, tool, max_turn = T.fib_dirs(70, 1.0), T.rod(5, 48, 2), 20000
    else:
        grid, dirs, tool = RR.box_scene(3, 24)
        dirs, max_turn = (dirs, -1) if which == "no_limit" else (dirs[2:3], 0)
    g = grid_of(ctx, grid)
    fit = g.torch_fit(dirs, tool, 1)
    if which == "no_obstacles":
        assert fit.n_free == g.n
    else:
        assert fit.n_free < g.n_free
    f = fit.occupancy()
    pts = [int(p) for p in np.flatnonzero(f)[np.linspace(0, int(f.sum()) - 1, 6).astype(np.int64)]]
    want = fit.geodesic_matrix(pts)
    assert (want > 0).any()
    assert np.array_equal(g.pose_matrix(dirs, tool, max_turn, pts), want)
    assert np.array_equal(g.pose_fields(dirs, tool, max_turn, pts[:2]), fit.geodesic_fields(pts[:2]))
    if which == "no_obstacles":
        assert np.array_equal(want, g.geodesic_matrix(pts))
    fit.close()
    g.close()


def test_two_calls_give_the_same_bytes(ctx):
    c = PR.box_case(3)
    g = grid_of(ctx, c["grid"])
    a = (c["dirs"], c["tool"], c["max_turn"])
    s, e, ps, pe = all_pairs(c["points"], c["pins"])
    one = [(digest(*g.pose_fields(*a, c["points"], c["pins"], states=True)), digest(g.pose_matrix(*a, c["points"], c["pins"])),
            digest(*[p for r in g.pose_paths(*a, s, e, ps, pe)[1:] for p in r if p is not None])) for _ in range(2)]
    assert one[0] == one[1]
    g.close()
