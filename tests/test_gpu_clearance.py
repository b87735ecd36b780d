"""GPU tests of obstacle clearance: wa_grid_distance_field, wa_grid_inflate and wa_traj_clearance through the C ABI against the
numpy restatements of tests/clearance_ref.py (which follow include/weldacs.h's definitions), bit for bit."""
import os

import numpy as np
import pytest

import clearance_ref as R
import pipeline_ref as PR
import waf
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, free, nx, ny, nz, cx=None, cy=None, cz=None, precision=1.0):
    ax = lambda n: np.arange(n, dtype=np.float32)
    return api.Grid.from_occupancy(ctx, free, ax(nx) if cx is None else cx, ax(ny) if cy is None else cy, ax(nz) if cz is None else cz,
                                   precision, 0)


@pytest.fixture(scope="module")
def cubic(ctx):
    """the cubic demo grid (main.cpp's cubic.stl at 0.0219, wall 8), its weld points and their voxels"""
    g = api.Grid.from_mesh(ctx, api.stl_read_file(os.path.join(G, "cubic.stl")), 0.0219, 8)
    pts = PR.read_points_file(os.path.join(G, "cubic_weld_points.in"))
    ids = g.resolve(pts)
    assert (ids >= 0).all()
    return g, ids


# ------------------------------------------------------------------ distance field
DIMS = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (63, 2, 3), (64, 3, 2), (65, 2, 3), (130, 3, 2), (7, 13, 11), (3, 65, 2),
        (2, 3, 64), (127, 1, 1), (5, 7, 3)]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("p", [0.0, 0.001, 0.1, 0.5, 1.0])
def test_edt_matches_brute_force(ctx, dims, p):
    nx, ny, nz = dims
    rs = np.random.RandomState(hash((dims, p)) & 0xFFFF)
    free = (rs.uniform(size=nx * ny * nz) >= p).astype(np.uint8)
    g = grid_of(ctx, free, nx, ny, nz)
    got = g.distance_field()
    want = R.edt_brute(free, nx, ny, nz)
    assert np.array_equal(got, want)
    if p == 0.0:
        assert (got == api.WA_D2_NONE).all()
    g.close()


def test_edt_single_obstacle_is_analytic(ctx):
    nx, ny, nz = 67, 45, 31
    free = np.ones(nx * ny * nz, np.uint8)
    o = (13, 40, 2)
    free[(o[2] * ny + o[1]) * nx + o[0]] = 0
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    want = ((xx - o[0]) ** 2 + (yy - o[1]) ** 2 + (zz - o[2]) ** 2).ravel()
    assert np.array_equal(grid_of(ctx, free, nx, ny, nz).distance_field(), want.astype(np.int32))


def test_edt_long_rows_and_the_int32_bound(ctx):
    n = 46341                       # (n - 1)^2 = 2 147 395 600 < 2^31: fits
    free = np.ones(n, np.uint8)
    free[0] = 0
    d = grid_of(ctx, free, n, 1, 1).distance_field()
    assert np.array_equal(d, (np.arange(n, dtype=np.int64) ** 2).astype(np.int32))
    free2 = np.ones(n + 1, np.uint8)   # 46341^2 >= 2^31: refused
    g = grid_of(ctx, free2, n + 1, 1, 1)
    with pytest.raises(api.WeldacsError) as e:
        g.distance_field()
    assert e.value.code == 1
    with pytest.raises(api.WeldacsError):
        g.inflate(1.0)


def _rows_with_gaps(nx):
    """occupied x per row (y = 0, 1) of a row of 6 chunks of 64 voxels and 5 more: where the row pass has to look ahead over chunks
    that hold no obstacle, or finds none at all"""
    return [("last partial chunk only", [[nx - 1, nx - 4], [nx - 5]]),
            ("chunks 0 and 5 only", [[3, 5 * 64 + 60], [63, 5 * 64]]),
            ("x = 63 and x = 64 only", [[63, 64], [63, 64]]),
            ("chunk 3 only", [[3 * 64, 3 * 64 + 63], [3 * 64 + 31]]),
            ("one row empty", [[], [10, 200, nx - 1]]),
            ("the other row empty", [[2 * 64 + 1, 4 * 64 + 63], []])]


@pytest.mark.parametrize("nz", [1, 2])
@pytest.mark.parametrize("case", _rows_with_gaps(64 * 6 + 5), ids=lambda c: c[0])
def test_edt_rows_with_empty_chunks(ctx, case, nz):
    nx, ny = 64 * 6 + 5, 2
    free = np.ones((nz, ny, nx), np.uint8)
    for y, xs in enumerate(case[1]):
        free[0, y, xs] = 0                                     # (nz = 2: layer 1 stays empty, its rows see only the layer below)
    free = free.ravel()
    g = grid_of(ctx, free, nx, ny, nz)
    assert np.array_equal(g.distance_field(), R.edt_brute(free, nx, ny, nz))
    g.close()


@pytest.mark.parametrize("n", [128, 256])
def test_edt_synth_grid_at_size(ctx, n):
    free, cx, cy, cz, p, wall = synth.synth_grid(n)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, p, wall)
    a = g.distance_field()
    assert np.array_equal(a, R.edt_separable(free, n, n, n))
    assert np.array_equal(g.distance_field(), a)          # cached: the same bits again
    assert np.array_equal(g.occupancy(), free)            # the input is not touched


def test_edt_stl_grid(ctx):
    v = waf.load(os.path.join(G, "vox_piece_p0148_w4.waf"))
    nx, ny, nz = (len(v["cx"]), len(v["cy"]), len(v["cz"]))
    free = np.unpackbits(v["free_packed"])[:nx * ny * nz]
    g = api.Grid.from_occupancy(ctx, free, v["cx"], v["cy"], v["cz"], float(v["precision"][0]), 4)
    a = g.distance_field()
    assert np.array_equal(a, R.edt_separable(free, nx, ny, nz))
    assert np.array_equal(a, g.distance_field())
    assert np.array_equal(g.occupancy(), free)


# ------------------------------------------------------------------ inflate
def test_inflate_radius0_is_the_input(ctx, cubic):
    g, ids = cubic
    z = g.inflate(0.0, ids)
    assert np.array_equal(z.occupancy(), g.occupancy()) and z.n_free == g.n_free
    assert (z.nx, z.ny, z.nz, z.wall) == (g.nx, g.ny, g.nz, g.wall) and z.precision == g.precision
    for a, b in zip(z.coords(), g.coords()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(g.inflate(0.0).occupancy(), g.occupancy())


def _pairs(ids):
    P = len(ids)
    return [(i, j) for i in range(P) for j in range(i + 1, P)]


def _solve_pairs(ctx, grid, ids):
    pairs = _pairs(ids)
    s = api.AcsSolver(ctx, grid, n_slots=len(pairs), max_colony=int(0.35 * 0.5 / 0.0219) + 1)
    p = api.default_params(max_iteration=150, predict=0.5, rng_mode=api.RNG_DEV, seed=2468)
    s.solve(p, [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs])
    out = [s.result(k)[:2] for k in range(len(pairs))]
    s.close()
    return out


def test_inflate_radius0_plans_the_same(ctx, cubic):
    g, ids = cubic
    a = _solve_pairs(ctx, g, ids)
    b = _solve_pairs(ctx, g.inflate(0.0, ids), ids)
    for (ca, pa), (cb, pb) in zip(a, b):
        assert np.float32(ca).view(np.uint32) == np.float32(cb).view(np.uint32) and np.array_equal(pa, pb)


@pytest.mark.parametrize("radius", [0.5, 1.0, 1.5, 2.0, 3.7])
def test_inflate_matches_restatement(ctx, radius):
    free, cx, cy, cz, p, wall = synth.synth_grid(64, seed=11, occ_prob=0.02)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, p, wall)
    keep = synth.synth_weld_points(free, 64, 12, seed=3)
    keep = np.concatenate([keep, [0, 64 ** 3 - 1]])           # bubbles clipped at the grid's corners
    got = g.inflate(radius, keep)
    want = R.inflate(free, g.distance_field(), 64, 64, 64, radius, keep)
    assert np.array_equal(got.occupancy(), want)
    assert got.n_free == int(want.sum())
    assert np.array_equal(g.occupancy(), free)                # g is not modified


def test_inflate_bad_arguments(ctx, cubic):
    g, ids = cubic
    occ = int(np.flatnonzero(g.occupancy() == 0)[0])
    for radius, keep in [(-1.0, None), (float("nan"), None), (float("inf"), None), (1.0, [occ]), (1.0, [-1]), (1.0, [g.n])]:
        with pytest.raises(api.WeldacsError) as e:
            g.inflate(radius, keep)
        assert e.value.code == 1


def test_inflated_plan_keeps_clearance(ctx, cubic):
    """radius 2 on the cubic demo with the weld points as keep ids: every pair stays reachable, every node of every path lies in a
    voxel free in the inflated grid, and outside the bubbles farther than 2 voxels from the metal"""
    g, ids = cubic
    r = 2.0
    gi = g.inflate(r, ids)
    assert gi.n_free < g.n_free
    d2 = g.distance_field()
    fi = gi.occupancy()
    nx, ny = g.nx, g.ny
    kx, ky, kz = ids % nx, (ids // nx) % ny, ids // (nx * ny)
    for (i, j), (cost, path) in zip(_pairs(ids), _solve_pairs(ctx, gi, ids)):
        assert len(path) >= 2 and path[0] == ids[i] and path[-1] == ids[j], (i, j, cost)
        path = path.astype(np.int64)
        assert (fi[path] == 1).all()
        px, py, pz = path % nx, (path // nx) % ny, path // (nx * ny)
        bub = (((px[:, None] - kx) ** 2 + (py[:, None] - ky) ** 2 + (pz[:, None] - kz) ** 2) <= (r + 1) ** 2).any(1)
        assert (d2[path[~bub]] > r * r).all()


# ------------------------------------------------------------------ trajectory check
def _check(ctx, g, free, xyz):
    cx, cy, cz = g.coords()
    t = api.Trajectory.from_points(ctx, np.asarray(xyz, np.float32).reshape(-1, 3))
    ids, d2, hit, s = t.clearance(g)
    wi, wd, wh, ws = R.clearance(free, g.distance_field(), g.nx, g.ny, g.nz, cx, cy, cz, xyz)
    assert np.array_equal(ids, wi) and np.array_equal(d2, wd) and np.array_equal(hit, wh) and s == ws, (s, ws)
    t.close()
    return s


def test_traj_hand_cases(ctx):
    nx = ny = nz = 5
    free = np.ones(125, np.uint8)
    free[(2 * ny + 2) * nx + 2] = 0                               # (2, 2, 2)
    g = grid_of(ctx, free, nx, ny, nz)
    # through the corner that the occupied voxel shares with three free ones: a hit
    s = _check(ctx, g, free, [[1, 2, 2], [2, 1, 2]])
    assert s["n_hit"] == 1 and s["first_hit"] == 0
    # beside it, along free voxels only: no hit
    s = _check(ctx, g, free, [[0, 0, 0], [4, 0, 0], [4, 4, 0], [4, 4, 4]])
    assert s["n_hit"] == 0 and s["first_hit"] == -1
    # samples outside the coordinate range, off-node coordinates, ties halfway between nodes, NaN
    s = _check(ctx, g, free, [[-3, 2, 2], [9, 2.5, 2.49], [2.5, 1.5, 0.5], [np.nan, 1, 1], [2, 2, 2]])
    assert s["n_outside"] == 3 and s["min_d2"] == 0 and s["argmin"] == 4
    s = _check(ctx, g, free, [[1.2, 3.9, 0.1]])                   # one sample: no segment
    assert s["n_hit"] == 0
    s = _check(ctx, g, free, np.zeros((0, 3)))                    # empty
    assert s == {"min_d2": api.WA_D2_NONE, "argmin": -1, "first_hit": -1, "n_hit": 0, "n_outside": 0}
    # no obstacle at all: every d2 is WA_D2_NONE
    g2 = grid_of(ctx, np.ones(125, np.uint8), nx, ny, nz)
    s = _check(ctx, g2, np.ones(125, np.uint8), [[0, 0, 0], [4, 4, 4]])
    assert s["min_d2"] == api.WA_D2_NONE and s["argmin"] == 0


def test_traj_random_vs_restatement(ctx):
    free, (nx, ny, nz), (cx, cy, cz), xyz = R.shuffled_scene()
    g = grid_of(ctx, free, nx, ny, nz, cx, cy, cz)
    s = _check(ctx, g, free, xyz)
    assert 0 < s["n_hit"] < len(xyz) - 1 and s["n_outside"] > 0


def test_stitched_paths_never_hit(ctx, cubic):
    """6-neighbour moves between free voxels: a stitched path's supercover is its own voxels, as long as every node maps back to
    itself -- which needs axis tables without a repeated coordinate"""
    g, ids = cubic
    for a in g.coords():
        assert len(np.unique(a)) == len(a)
    gi = g.inflate(2.0, ids)
    for grid in (g, gi):
        for _, path in _solve_pairs(ctx, grid, ids):
            tids, d2, hit, s = api.Trajectory.stitch(grid, [path]).clearance(grid)
            assert np.array_equal(tids, path.astype(np.int64))
            assert s["n_hit"] == 0 and s["n_outside"] == 0 and s["min_d2"] >= 1


def test_smoothed_trajectory_vs_restatement(ctx, cubic):
    """the two-pass B-spline output of main.cpp's cubic demo (golden): per-sample and per-segment outputs equal the restatement;
    whether the smoothed curve cuts the grid is recorded, not asserted"""
    g, _ = cubic
    sm = waf.load(os.path.join(G, "smooth_cubic_fill0.waf"))
    xyz = sm["s2_samples"].reshape(-1, 3)
    s = _check(ctx, g, g.occupancy(), xyz)
    print("[clearance] smoothed cubic trajectory: %d samples, summary %s, min clearance %.4f m"
          % (len(xyz), s, np.sqrt(s["min_d2"]) * float(g.precision)))
