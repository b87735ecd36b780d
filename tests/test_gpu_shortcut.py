"""GPU tests of wa_grid_path_shortcut: waypoints and lengths through the C ABI against the numpy restatement of tests/shortcut_ref.py (which
follows include/weldacs.h's definition), bit for bit; refusals; and the shortened plans of the cubic demo and of plan_batch.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pipeline_ref as PR
import shortcut_ref as S
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, free, nx, ny, nz, cx=None, cy=None, cz=None):
    ax = lambda n: np.arange(n, dtype=np.float32)
    return api.Grid.from_occupancy(ctx, free, ax(nx) if cx is None else cx, ax(ny) if cy is None else cy, ax(nz) if cz is None else cz,
                                   1.0, 0)


def _same(ctx, g, free, paths, span, cache=None):
    """one batched call against the restatement, path by path: waypoint node ids and float64 length bits"""
    cx, cy, cz = g.coords()
    wps, lengths = api.shortcut_paths(g, paths, span)
    assert len(wps) == len(paths) and lengths.dtype == np.float64
    for p, w, ln in zip(paths, wps, lengths):
        p = np.asarray(p, np.int64)
        if len(p) == 0:
            assert len(w) == 0 and ln == 0.0
            continue
        ww, wl = S.shortcut(free, g.nx, g.ny, cx, cy, cz, p, span, cache)
        assert np.array_equal(w, p[ww]), (span, len(p))
        assert np.float64(ln).view(np.uint64) == np.float64(wl).view(np.uint64), (span, len(p), ln, wl)
    return wps, lengths


@pytest.mark.parametrize("case", S.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    name, free, (nx, ny, nz), path, span, want = case
    g = grid_of(ctx, free, nx, ny, nz)
    wps, _ = _same(ctx, g, free, [path], span)
    assert wps[0].tolist() == [path[k] for k in want]
    w, ln = g.shortcut(path, span)
    assert w.tolist() == wps[0].tolist()


def _walk(rs, free, dims, L, nb, start=None):
    """a random walk of L nodes with 6- or 26-neighbour steps (kept inside the grid), through occupied voxels too"""
    nx, ny, nz = dims
    steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] if nb == 6 else \
        [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    p = np.array(start if start is not None else [rs.randint(nx), rs.randint(ny), rs.randint(nz)])
    out = []
    for _ in range(L):
        out.append((p[2] * ny + p[1]) * nx + p[0])
        p = np.clip(p + np.array(steps[rs.randint(len(steps))]), 0, [nx - 1, ny - 1, nz - 1])
    return np.array(out, np.int64)


@pytest.mark.parametrize("occ", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("nb", [6, 26])
def test_random_grids_and_paths(ctx, occ, nb):
    rs = np.random.RandomState(int(occ * 100) + nb)
    dims = (11, 9, 7)
    nx, ny, nz = dims
    free = (rs.uniform(size=nx * ny * nz) >= occ).astype(np.uint8)
    # non-uniform fp32 tables: the lengths are not sums of small integers
    cx = np.cumsum(rs.uniform(0.01, 0.05, nx)).astype(np.float32)
    cy = np.cumsum(rs.uniform(0.01, 0.05, ny)).astype(np.float32)
    cz = (np.cumsum(rs.uniform(0.01, 0.05, nz)) - 0.1).astype(np.float32)
    g = grid_of(ctx, free, nx, ny, nz, cx, cy, cz)
    paths = [_walk(rs, free, dims, L, nb) for L in (1, 2, 64, 65, 2000)]
    batch = [paths[0], np.zeros(0, np.int64), paths[1], paths[2], np.zeros(0, np.int64), paths[3], paths[4], np.zeros(0, np.int64)]
    cache = {}
    for span in (1, 63, 64, 65, 128, 4096):
        wps, lengths = _same(ctx, g, free, batch, span, cache)
        if span == 1:
            for p, w in zip(batch, wps):
                assert np.array_equal(w, p)
    assert len(cache) > 0


def test_long_straight_path_crosses_chunks(ctx):
    """an open row of 300 voxels: one wave tests 64 candidates per chunk, so spans 63..65, 128 and 4096 end in every chunk position"""
    n = 300
    free = np.ones(n * 2, np.uint8)
    g = grid_of(ctx, free, n, 2, 1)
    path = np.arange(n, dtype=np.int64)
    for span, want in [(63, list(range(0, n - 1, 63)) + [n - 1]), (64, list(range(0, n - 1, 64)) + [n - 1]),
                       (65, list(range(0, n - 1, 65)) + [n - 1]), (128, [0, 128, 256, n - 1]), (4096, [0, n - 1])]:
        wps, lengths = _same(ctx, g, free, [path], span)
        assert wps[0].tolist() == want
        assert lengths[0] == float(n - 1)
    # an obstacle beside the row, one step off it: the detour sees past it only where the cover clears it
    free2 = free.copy()
    free2[n + 150] = 0                                            # (150, 1)
    g2 = grid_of(ctx, free2, n, 2, 1)
    det = np.concatenate([np.arange(0, 140), n + np.arange(140, 148), np.arange(148, n)]).astype(np.int64)
    _same(ctx, g2, free2, [det, path], 4096)


def test_batch_equals_single_calls(ctx):
    rs = np.random.RandomState(5)
    dims = (16, 12, 10)
    free = (rs.uniform(size=int(np.prod(dims))) >= 0.15).astype(np.uint8)
    g = grid_of(ctx, free, *dims)
    paths = [_walk(rs, free, dims, int(L), nb) for L, nb in zip(rs.randint(0, 400, 40), [6, 26] * 20)]
    wps, lengths = api.shortcut_paths(g, paths, 128)
    for p, w, ln in zip(paths, wps, lengths):
        w1, l1 = api.shortcut_paths(g, [p], 128)
        assert np.array_equal(w1[0], w) and np.float64(l1[0]).view(np.uint64) == np.float64(ln).view(np.uint64)
    # the rest of each path's range in the caller's buffer is left as it was
    ids = np.concatenate(paths)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    wp = np.full(len(ids), -7, np.int64)
    cnt = np.zeros(len(paths), np.int32)
    assert ctx.lib.wa_grid_path_shortcut(g.h, ids.ctypes.data, off.ctypes.data, len(paths), 128, wp.ctypes.data, cnt.ctypes.data, None) == 0
    for k, p in enumerate(paths):
        seg = wp[off[k]:off[k + 1]]
        assert np.array_equal(p[seg[:cnt[k]]], wps[k]) and (seg[cnt[k]:] == -7).all()


@pytest.mark.parametrize("n_paths", [255, 256, 257, 513])
def test_more_paths_than_one_block(ctx, n_paths):
    """k_sc_chain runs one lane per path: batches either side of one and two blocks of 256 lanes, empty paths among them"""
    rs = np.random.RandomState(n_paths)
    dims = (16, 12, 10)
    free = (rs.uniform(size=int(np.prod(dims))) >= 0.15).astype(np.uint8)
    g = grid_of(ctx, free, *dims)
    lens = rs.randint(0, 41, n_paths)
    lens[[0, 63, 64, n_paths - 2]] = 0                            # empty paths at a wave's edges and next to the last lane
    lens[[255, n_paths - 1] if n_paths > 255 else [n_paths - 1]] = 40
    paths = [_walk(rs, free, dims, int(ln), nb) for ln, nb in zip(lens, [6, 26] * n_paths)]
    assert len(paths) == n_paths and sum(len(p) == 0 for p in paths) >= 4
    wps, _ = _same(ctx, g, free, paths, 128, {})
    assert any(0 < len(w) < len(p) for p, w in zip(paths[256:], wps[256:])) or n_paths <= 256   # something shortened behind block 0


def test_refusals(ctx):
    n = 6
    g = grid_of(ctx, np.ones(n ** 3, np.uint8), n, n, n)
    ids = np.array([0, 1, 2, 3], np.int64)
    off = np.array([0, 2, 4], np.int64)
    wp, cnt, ln = np.zeros(4, np.int64), np.zeros(2, np.int32), np.zeros(2, np.float64)
    f = ctx.lib.wa_grid_path_shortcut
    P = lambda a: a.ctypes.data

    def call(g_=g.h, ids_=ids, off_=off, n_=2, span=8, wp_=wp, cnt_=cnt):
        return f(g_, P(ids_) if ids_ is not None else None, P(off_) if off_ is not None else None, n_, span,
                 P(wp_) if wp_ is not None else None, P(cnt_) if cnt_ is not None else None, P(ln))

    assert call() == 0 and cnt.tolist() == [2, 2]
    bad = [dict(g_=None), dict(ids_=None), dict(off_=None), dict(wp_=None), dict(cnt_=None), dict(n_=-1), dict(span=0),
           dict(span=4097), dict(off_=np.array([0, 3, 2], np.int64)), dict(off_=np.array([1, 2, 4], np.int64)),
           dict(ids_=np.array([0, 1, -1, 3], np.int64)), dict(ids_=np.array([0, 1, n ** 3, 3], np.int64))]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(span=1) == 0 and call(span=4096) == 0
    assert call(n_=0) == 0                                        # no paths: nothing to do


# ------------------------------------------------------------------ the cubic demo, planned on the radius-2 inflated grid
def _pairs(ids):
    P = len(ids)
    return [(i, j) for i in range(P) for j in range(i + 1, P)]


def _solve_pairs(ctx, grid, ids):
    pairs = _pairs(ids)
    s = api.AcsSolver(ctx, grid, n_slots=len(pairs), max_colony=int(0.35 * 0.5 / 0.0219) + 1)
    p = api.default_params(max_iteration=150, predict=0.5, rng_mode=api.RNG_DEV, seed=2468)
    s.solve(p, [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs])
    costs, paths = s.results(len(pairs))
    s.close()
    return list(zip(costs, paths))


def test_cubic_demo_shortened_plans_keep_clearance(ctx):
    g = api.Grid.from_mesh(ctx, api.stl_read_file(os.path.join(G, "cubic.stl")), 0.0219, 8)
    ids = g.resolve(PR.read_points_file(os.path.join(G, "cubic_weld_points.in")))
    assert (ids >= 0).all()
    for a in g.coords():
        assert len(np.unique(a)) == len(a)                        # every node maps back to itself (see test_gpu_clearance.py)
    gi = g.inflate(2.0, ids)
    paths = [np.asarray(p, np.int64) for _, p in _solve_pairs(ctx, gi, ids)]
    wps, lengths = api.shortcut_paths(gi, paths, 128)
    _, lattice = api.shortcut_paths(gi, paths, 1)
    shorter = 0
    for p, w, ln, lat in zip(paths, wps, lengths, lattice):
        assert len(p) >= 2 and w[0] == p[0] and w[-1] == p[-1]
        s = api.Trajectory.stitch(gi, [w]).clearance(gi)[3]
        assert s["n_hit"] == 0 and s["n_outside"] == 0
        assert ln <= lat * (1 + 1e-12)
        shorter += ln < lat
    assert shorter >= 1
    print("[shortcut] cubic demo, radius 2: %d pairs, %d shortened, waypoints %d of %d nodes, length %.4f of %.4f m"
          % (len(paths), shorter, sum(len(w) for w in wps), sum(len(p) for p in paths), lengths.sum(), lattice.sum()))


def test_plan_batch_shortcut(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "96", "--points", "16", "--shortcut",
           "--clearance", "0.02"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["all_reached"]
    assert out["shortened_length_total"] < out["lattice_length_total"]
    assert out["waypoints"] >= 2 and "trajectory_clearance" in out
    print("[shortcut] plan_batch:", {k: out[k] for k in ("tour_cost", "shortened_length_total", "lattice_length_total", "waypoints",
                                                        "shortcut_smoothing", "trajectory_clearance") if k in out})
