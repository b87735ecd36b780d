"""GPU tests of the exact shortest-path fields (wa_grid_geodesic_fields / _matrix / _paths) through the C ABI against the numpy
restatement of tests/geodesic_ref.py (which follows include/weldacs.h's definition).  Hop counts are integers: every comparison is an
equality (np.array_equal), there is no tolerance anywhere in this file."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import geodesic_ref as G
import limit_ref as R
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ARG, CAPACITY = 1, 7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, free, dims):
    ax = lambda n: np.arange(n, dtype=np.float32)
    return api.Grid.from_occupancy(ctx, free, ax(dims[0]), ax(dims[1]), ax(dims[2]), 1.0, 0)


def vid(dims, x, y, z):
    return x + dims[0] * (y + dims[1] * z)


# ------------------------------------------------------------------ 1. fields on random boxes whose x size covers word edges
def random_box(dims, occ, seed):
    """seeded occupancy with, where the box has room, a free voxel enclosed by its occupied neighbours (a pocket of one voxel) at the
    centre; returns (free, sources): corners, the pocket and a few random free voxels"""
    nx, ny, nz = dims
    n = nx * ny * nz
    rs = np.random.RandomState(seed)
    free = (rs.uniform(size=n) >= occ).astype(np.uint8)
    srcs = []
    for x, y, z in ((0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, 0), (0, ny - 1, nz - 1)):
        free[vid(dims, x, y, z)] = 1
        srcs.append(vid(dims, x, y, z))
    c = (nx // 2, ny // 2, nz // 2)
    p = vid(dims, *c)
    free[p] = 1
    for v in G.neighbours(p, dims):
        free[v] = 0
    for x, y, z in ((0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, 0), (0, ny - 1, nz - 1)):
        free[vid(dims, x, y, z)] = 1     # (a box of one or two voxels across: the corners win over the pocket's shell)
    srcs.append(p)
    cand = np.flatnonzero(free)
    srcs += [int(v) for v in cand[rs.randint(len(cand), size=3)]]
    return free, list(dict.fromkeys(srcs))


BOXES = [((1, 1, 1), 0.1), ((1, 7, 5), 0.1), ((63, 1, 1), 0.1), ((63, 5, 4), 0.3), ((64, 3, 1), 0.1), ((64, 6, 5), 0.45), ((65, 1, 7), 0.3),
         ((65, 5, 3), 0.45), ((127, 2, 2), 0.1), ((127, 4, 6), 0.45), ((130, 3, 3), 0.3), ((130, 7, 4), 0.45), ((130, 1, 1), 0.1),
         ((1, 1, 9), 0.3), ((64, 1, 1), 0.45)]


@pytest.mark.parametrize("dims,occ", BOXES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fields_on_random_boxes(ctx, dims, occ):
    free, srcs = random_box(dims, occ, seed=dims[0] * 1000 + dims[1] * 10 + dims[2])
    g = grid_of(ctx, free, dims)
    got = g.geodesic_fields(srcs)
    want = G.fields(free, dims, srcs)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    if occ >= 0.45 and np.prod(dims) > 500:
        assert (want[0][free != 0] == G.NONE).mean() > 0.02, "the dense boxes are there for their unreachable voxels"
    m = g.geodesic_matrix(srcs)
    assert np.array_equal(m, want[:, srcs])
    g.close()


def test_fields_do_not_depend_on_the_chunking(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a child process) and all in one launch"""
    dims = (70, 9, 6)
    free, srcs = random_box(dims, 0.3, seed=5)
    g = grid_of(ctx, free, dims)
    whole = g.geodesic_fields(srcs)
    g.close()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "import numpy as np, hashlib\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_geodesic import random_box, grid_of\n"
             "free, srcs = random_box((70, 9, 6), 0.3, seed=5)\n"
             "c = api.Context(0); g = grid_of(c, free, (70, 9, 6))\n"
             "print('digest', hashlib.blake2b(g.geodesic_fields(srcs).tobytes(), digest_size=16).hexdigest(),"
             " hashlib.blake2b(g.geodesic_matrix(srcs).tobytes(), digest_size=16).hexdigest())\n" % (ROOT, os.path.join(ROOT, "tests")))
    import hashlib
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    assert line[1] == hashlib.blake2b(whole.tobytes(), digest_size=16).hexdigest()
    assert line[2] == hashlib.blake2b(np.ascontiguousarray(whole[:, srcs]).tobytes(), digest_size=16).hexdigest()


# ------------------------------------------------------------------ 2. the benchmark grid
def _row_128(i):
    """worker: the restatement's field of weld point i on synth_grid(128), as (its values at the 64 points, the whole field for 3 of them)"""
    free = synth.synth_grid(128)[0]
    pts = synth.synth_weld_points(free, 128, 64)
    f = G.field(free, (128, 128, 128), pts[i])
    return f[pts], (f if i in (0, 31, 63) else None)


def test_matrix_synth_128(ctx):
    """all 64 rows against the restatement (64 numpy searches of a few seconds each, in worker processes)"""
    import concurrent.futures as cf
    import multiprocessing as mp
    n = 128
    free = synth.synth_grid(n)[0]
    pts = synth.synth_weld_points(free, n, 64)
    with cf.ProcessPoolExecutor(min(16, os.cpu_count() or 1), mp_context=mp.get_context("spawn")) as pool:
        jobs = pool.map(_row_128, range(64))
        g = grid_of(ctx, free, (n, n, n))
        m = g.geodesic_matrix(pts)
        f = g.geodesic_fields(pts)
        g.close()
        res = list(jobs)
    assert m.shape == (64, 64) and np.array_equal(m, m.T) and (np.diag(m) == 0).all() and (m != G.NONE).all()
    assert np.array_equal(m, np.stack([r[0] for r in res]))
    for i in (0, 31, 63):
        assert np.array_equal(f[i], res[i][1])
    assert np.array_equal(f[:, pts], m), "fields and matrix are two routes to the same numbers"


# ------------------------------------------------------------------ 3. hops far from Manhattan
@pytest.mark.parametrize("dims,every", [((40, 9, 7), 3), ((131, 6, 5), 4), ((66, 12, 3), 2)])
def test_baffles(ctx, dims, every):
    free = G.baffles(*dims, every=every)
    g = grid_of(ctx, free, dims)
    n = int(np.prod(dims))
    cand = np.flatnonzero(free)
    pts = [0, n - 1 if free[n - 1] else int(cand[-1])] + [int(v) for v in cand[np.random.RandomState(3).randint(len(cand), size=6)]]
    want = G.fields(free, dims, pts)
    man = abs(np.array(np.unravel_index(pts[1], dims[::-1])) - 0).sum()
    assert want[0][pts[1]] > 2 * man, "the baffles make the way several times the Manhattan distance"
    assert np.array_equal(g.geodesic_fields(pts), want)
    assert np.array_equal(g.geodesic_matrix(pts), want[:, pts])
    g.close()


# ------------------------------------------------------------------ 4. more than 65 535 levels
SERPENTINE = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import geodesic_ref as G
from welding_robot_amd import api
nx, ny = 1100, 130
dims = (nx, ny, 1)
free = G.serpentine(nx, ny)
n_free = int(free.sum())
assert n_free == 65 * nx + 65 and n_free - 1 > 65535
ctx = api.Context(0)
ax = lambda n: np.arange(n, dtype=np.float32)
g = api.Grid.from_occupancy(ctx, free, ax(nx), ax(ny), ax(1), 1.0, 0)
f = g.geodesic_fields([0])[0]
assert f.max() == n_free - 1, (int(f.max()), n_free - 1)
assert np.array_equal(f >= 0, free != 0)
assert np.array_equal(np.sort(f[free != 0]), np.arange(n_free, dtype=np.int32)), "one voxel per level"
far = int(np.argmax(f))
assert far == (nx - 1) + nx * (ny - 1), "the gap of the last wall row"
mid = 5 + nx * 64
m = g.geodesic_matrix([0, far, mid])
assert m[0, 1] == m[1, 0] == n_free - 1 and m[0, 2] == m[2, 0] == f[mid] and m[1, 2] == n_free - 1 - f[mid]
hops, paths = api.geodesic_paths(g, [0, far], [far, mid])
assert hops.tolist() == [n_free - 1, n_free - 1 - int(f[mid])] and len(paths[0]) == n_free
G.check_path(free, dims, paths[0], 0, far, n_free - 1)
G.check_path(free, dims, paths[1], far, mid, int(hops[1]))
assert np.array_equal(f[paths[0]], np.arange(n_free, dtype=np.int32))
print("serpentine ok", n_free - 1, flush=True)
'''


def test_serpentine_beyond_16_bits():
    """1100 x 130 x 1, a wall on every second row with its gap at alternating ends: 65 corridors of 1100 voxels and 65 gaps, 71 565
    free voxels in one line, so the far end is 71 564 hops away: the exact count there (the level counter must not be 16 bits wide), one
    voxel per level, and the path is the whole line.  The host reads one word per source every 32 levels, about 2 240 round trips.  No
    assertion on time: the child process has a time limit of its own."""
    r = subprocess.run([sys.executable, "-c", SERPENTINE % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "serpentine ok 71564" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------ 5. paths
def _raw_paths(ctx, g, starts, ends, off, ids, hops):
    return ctx.lib.wa_grid_geodesic_paths(g.h, starts.ctypes.data, ends.ctypes.data, len(starts), off.ctypes.data, ids.ctypes.data, hops.ctypes.data)


def test_paths_against_the_restatement(ctx):
    dims = (67, 11, 9)
    free, _ = random_box(dims, 0.3, seed=77)
    pocket = vid(dims, dims[0] // 2, dims[1] // 2, dims[2] // 2)
    rs = np.random.RandomState(4)
    cand = np.flatnonzero(free)
    want_f = G.field(free, dims, 0)
    reach = np.flatnonzero(want_f >= 0)
    s_pool = [0] + [int(v) for v in reach[rs.randint(len(reach), size=5)]]
    starts = [s_pool[k] for k in rs.randint(len(s_pool), size=40)]           # repeated starts, in no order
    ends = [int(v) for v in cand[rs.randint(len(cand), size=40)]]
    starts[7], ends[7] = s_pool[2], s_pool[2]                                # start == end
    starts[20], ends[20] = s_pool[1], pocket                                 # unreachable, in the middle of the batch
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    g = grid_of(ctx, free, dims)
    w_hops, w_paths = G.paths(free, dims, starts, ends)
    assert w_hops[20] == G.NONE and w_hops[7] == 0 and (w_hops > 20).sum() > 5
    hops, paths = api.geodesic_paths(g, starts, ends)
    assert np.array_equal(hops, w_hops)
    for k in range(40):
        if w_hops[k] < 0:
            assert paths[k] is None
            continue
        assert np.array_equal(paths[k], w_paths[k]), k
        G.check_path(free, dims, paths[k], int(starts[k]), int(ends[k]), int(hops[k]))   # independent of the restatement
    # the raw call: ranges with slack, a sentinel everywhere, nothing written behind a path or into the unreachable pair's range
    SENT = -77
    cap = np.maximum(w_hops.astype(np.int64) + 1, 0) + 3
    off = np.concatenate([[5], 5 + np.cumsum(cap)]).astype(np.int64)
    ids = np.full(int(off[-1]) + 4, SENT, np.int64)
    h2 = np.full(40, SENT, np.int32)
    assert _raw_paths(ctx, g, starts, ends, off, ids, h2) == 0
    assert np.array_equal(h2, w_hops)
    assert (ids[:5] == SENT).all() and (ids[off[-1]:] == SENT).all()
    for k in range(40):
        L = max(int(w_hops[k]) + 1, 0)
        if L:
            assert np.array_equal(ids[off[k]:off[k] + L], w_paths[k])
        assert (ids[off[k] + L:off[k + 1]] == SENT).all(), k
    # the capacity round trip: one reachable pair one id short
    k_short = int(np.argmax(w_hops))
    cap2 = np.maximum(w_hops.astype(np.int64) + 1, 0)
    cap2[k_short] -= 1
    off2 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids2 = np.full(int(off2[-1]) + 1, SENT, np.int64)
    h3 = np.full(40, SENT, np.int32)
    assert _raw_paths(ctx, g, starts, ends, off2, ids2, h3) == CAPACITY
    assert np.array_equal(h3, w_hops), "hops_out is filled for every pair, also on WA_ERR_CAPACITY"
    assert (ids2[off2[k_short]:off2[k_short + 1]] == SENT).all(), "nothing is written for the pair that does not fit"
    for k in range(40):
        if k != k_short and w_hops[k] >= 0:
            assert np.array_equal(ids2[off2[k]:off2[k + 1]], w_paths[k])
    cap2[k_short] += 1                                                       # sized from hops_out: the second call succeeds
    off3 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids3 = np.full(int(off3[-1]) + 1, SENT, np.int64)
    assert _raw_paths(ctx, g, starts, ends, off3, ids3, h3) == 0
    assert np.array_equal(ids3[off3[k_short]:off3[k_short + 1]], w_paths[k_short])
    g.close()


def test_paths_tie_and_baffles(ctx):
    free, dims, s, e, want = G.tie_case()
    g = grid_of(ctx, free, dims)
    hops, paths = api.geodesic_paths(g, [s, e, s], [e, s, s])
    assert hops.tolist() == [3, 3, 0] and paths[0].tolist() == want and paths[1].tolist() == [7, 3, 1, 0] and paths[2].tolist() == [0]
    g.close()
    dims = (40, 9, 7)
    free = G.baffles(*dims)
    g = grid_of(ctx, free, dims)
    n = int(np.prod(dims))
    starts, ends = [0, n - 1, 0, 200], [n - 1, 0, 200, n - 1]
    hops, paths = api.geodesic_paths(g, starts, ends)
    w_hops, w_paths = G.paths(free, dims, starts, ends)
    assert np.array_equal(hops, w_hops)
    for a, b in zip(paths, w_paths):
        assert np.array_equal(a, b)
    g.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments(ctx):
    dims = (9, 4, 3)
    free = np.ones(108, np.uint8)
    free[50] = 0
    g = grid_of(ctx, free, dims)
    lib = ctx.lib
    SENT = -77
    hops = np.full(4 * 108, SENT, np.int32)
    ids_out = np.full(64, SENT, np.int64)
    off = np.array([0, 30, 60], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ok_ids = i64(0, 107)

    def untouched():
        return (hops == SENT).all() and (ids_out == SENT).all()

    for bad in (i64(0, 50), i64(0, 108), i64(-1, 0), i64(0, 1 << 40)):       # occupied, outside (above, below, far above)
        assert lib.wa_grid_geodesic_fields(g.h, bad.ctypes.data, 2, hops.ctypes.data) == ARG and untouched()
        if bad[1] == 50:
            assert b"occupied" in lib.wa_last_error(ctx.h)
        assert lib.wa_grid_geodesic_matrix(g.h, bad.ctypes.data, 2, hops.ctypes.data) == ARG and untouched()
        assert lib.wa_grid_geodesic_paths(g.h, bad.ctypes.data, ok_ids.ctypes.data, 2, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, bad.ctypes.data, 2, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
        assert untouched()
    # negative counts, NULL arrays (also with a count of 0), NULL outputs, decreasing offsets
    assert lib.wa_grid_geodesic_fields(g.h, ok_ids.ctypes.data, -1, hops.ctypes.data) == ARG
    assert lib.wa_grid_geodesic_matrix(g.h, ok_ids.ctypes.data, -1, hops.ctypes.data) == ARG
    assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, ok_ids.ctypes.data, -1, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
    for cnt in (0, 2):
        assert lib.wa_grid_geodesic_fields(g.h, None, cnt, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_matrix(g.h, None, cnt, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_fields(g.h, ok_ids.ctypes.data, cnt, None) == ARG
        assert lib.wa_grid_geodesic_matrix(g.h, ok_ids.ctypes.data, cnt, None) == ARG
        assert lib.wa_grid_geodesic_paths(g.h, None, ok_ids.ctypes.data, cnt, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, None, cnt, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, ok_ids.ctypes.data, cnt, None, ids_out.ctypes.data, hops.ctypes.data) == ARG
        assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, ok_ids.ctypes.data, cnt, off.ctypes.data, ids_out.ctypes.data, None) == ARG
    down = np.array([0, 30, 29], np.int64)
    assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, ok_ids.ctypes.data, 2, down.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == ARG
    assert untouched()
    # counts of zero with valid pointers succeed and write nothing
    assert lib.wa_grid_geodesic_fields(g.h, ok_ids.ctypes.data, 0, hops.ctypes.data) == 0
    assert lib.wa_grid_geodesic_matrix(g.h, ok_ids.ctypes.data, 0, hops.ctypes.data) == 0
    assert lib.wa_grid_geodesic_paths(g.h, ok_ids.ctypes.data, ok_ids.ctypes.data, 0, off.ctypes.data, ids_out.ctypes.data, hops.ctypes.data) == 0
    assert untouched()
    # and the grid is as it was
    assert np.array_equal(g.occupancy(), free)
    assert g.geodesic_matrix(ok_ids).tolist() == [[0, 8 + 3 + 2], [8 + 3 + 2, 0]]
    g.close()


# ------------------------------------------------------------------ 7. against the solver
def test_colony_paths_are_never_shorter_and_of_the_same_parity(ctx):
    """synth_grid(96), 16 weld points, the defaults of examples/plan_batch.py (150 generations, 24 ants, seed 7, WA_RNG_DEV, stream =
    global pair index): every one of the 120 best paths is a lattice path between the two points, so it has at least hops steps, and the
    lattice is bipartite, so the excess is even.  The test counts what it compared: a solver that found nothing fails it."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import plan_batch
    n, P = 96, 16
    free, cx, cy, cz, prec, wall = synth.synth_grid(n)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, P, seed=7)
    cost, paths, _ = plan_batch.plan(ctx, g, pts, 150, float(0.35 ** -1 * 24), 7, 0)
    m = g.geodesic_matrix(pts)
    assert (m >= 0).all()
    compared = at_optimum = 0
    for (i, j), ids in paths.items():
        if not np.isfinite(cost[i, j]):
            continue
        assert ids[0] == pts[i] and ids[-1] == pts[j]
        steps = len(ids) - 1
        assert steps >= m[i, j] and (steps - m[i, j]) % 2 == 0, (i, j, steps, int(m[i, j]))
        compared += 1
        at_optimum += steps == m[i, j]
    print("colony searches at the optimum: %d of %d" % (at_optimum, compared))
    assert compared == 120
    g.close()


# ------------------------------------------------------------------ 8. a weld point cut off by the inflation
def test_inflated_grid_with_a_cut_off_point(ctx):
    """20 x 12 x 12: metal fills x >= 8 except a corridor one voxel wide along x at (y, z) = (6, 6) from the face to the weld point A =
    (15, 6, 6).  Inflating by 1 voxel closes the corridor (every voxel of it touches metal) except within 2 voxels of A, where the keep
    bubble leaves the grid as it was: A keeps a pocket of three voxels and no way out."""
    dims = (20, 12, 12)
    f3 = np.ones((12, 12, 20), np.uint8)
    f3[:, :, 8:] = 0
    f3[6, 6, 8:16] = 1
    free = f3.reshape(-1)
    A = vid(dims, 15, 6, 6)
    pts = np.array([vid(dims, 2, 2, 2), vid(dims, 3, 8, 5), A, vid(dims, 1, 5, 9)], np.int64)
    metal = grid_of(ctx, free, dims)
    m0 = metal.geodesic_matrix(pts)
    assert (m0 >= 0).all() and m0[0, 2] == 13 + 4 + 4
    plan = metal.inflate(1.0, pts)
    pf = plan.occupancy()
    m = plan.geodesic_matrix(pts)
    assert np.array_equal(m, G.matrix(pf, dims, pts))
    assert m[2].tolist() == [G.NONE, G.NONE, 0, G.NONE] and m[:, 2].tolist() == [G.NONE, G.NONE, 0, G.NONE]
    others = [0, 1, 3]
    assert (m[np.ix_(others, others)] >= 0).all()
    f = plan.geodesic_fields([A])[0]
    assert (f >= 0).sum() == 3
    s = api.AcsSolver(ctx, plan, n_slots=1, max_colony=8)
    s.solve(api.default_params(max_iteration=20, predict=8 / 0.35, fixed_colony=8, rng_mode=api.RNG_DEV, seed=1), pts[0], A)
    assert s.result()[0] == np.inf
    s.close()
    plan.close()
    metal.close()


# ------------------------------------------------------------------ 9. full size
def test_matrix_c5_full_size(ctx):
    """256^3 synth_grid, C5's 64 weld points, matrix only.  Rows of 4 sources against the restatement's, which tests/golden/
    geodesic_c5_rows.json holds (python tests/geodesic_ref.py writes it: its numpy search costs about 0.2 s a level at this size)."""
    gold = json.load(open(os.path.join(GOLD, "geodesic_c5_rows.json")))
    assert gold["grid"] == 256 and gold["points"] == 64 and gold["sources"] == list(G.GOLDEN_256_SOURCES)
    n = 256
    free = synth.synth_grid(n)[0]
    pts = synth.synth_weld_points(free, n, 64)
    g = grid_of(ctx, free, (n, n, n))
    m = g.geodesic_matrix(pts)
    assert np.array_equal(m, m.T) and (np.diag(m) == 0).all() and (m >= 0).all()
    assert np.array_equal(m[gold["sources"]], np.array(gold["rows"], np.int32))
    g.close()


def test_one_source_at_the_solvers_limit(ctx):
    """2^27 voxels (512^3, limit_ref.box_free at 10 %), one source.  Which voxels are reachable: scipy.ndimage.label.  The counts: exact
    at EVERY voxel, not a sample, by the local conditions of geodesic_ref.bellman_exact (tests/test_geodesic_rules.py checks the
    checker), which only the true field satisfies; plus the Manhattan
    distance as a lower bound and equality along the free run of voxels in front of the source."""
    from scipy import ndimage
    dims = (512, 512, 512)
    src = vid(dims, 17, 300, 255)
    free = R.box_free(dims, 11, 0.10, [src])
    g = grid_of(ctx, free, dims)
    hops = g.geodesic_fields([src])[0]
    g.close()
    lab, _ = ndimage.label(free.reshape(512, 512, 512) != 0)
    lab = lab.reshape(-1)
    assert np.array_equal(hops >= 0, lab == lab[src])
    del lab
    assert G.bellman_exact(hops, free, dims, src)
    sample = np.random.RandomState(0).randint(len(free), size=100000)
    sample = sample[hops[sample] >= 0]
    z, y, x = np.unravel_index(sample, (512, 512, 512))
    assert (hops[sample] >= abs(x - 17) + abs(y - 300) + abs(z - 255)).all()
    run = 0
    while free[src + run + 1]:
        run += 1
        assert hops[src + run] == run


# ------------------------------------------------------------------ 10. repeatability, two contexts
def test_same_bytes_twice_and_two_contexts(ctx):
    dims = (130, 20, 12)
    free, srcs = random_box(dims, 0.3, seed=9)
    other = api.Context(0)
    dims2 = (65, 9, 9)
    free2 = G.baffles(*dims2)
    g, g2 = grid_of(ctx, free, dims), grid_of(other, free2, dims2)
    pts2 = [0, int(np.prod(dims2)) - 1, 300]
    a = g.geodesic_fields(srcs)
    b2 = g2.geodesic_fields(pts2)
    b = g.geodesic_fields(srcs)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, G.fields(free, dims, srcs)) and np.array_equal(b2, G.fields(free2, dims2, pts2))
    m1, m2 = g.geodesic_matrix(srcs), g2.geodesic_matrix(pts2)
    assert m1.tobytes() == g.geodesic_matrix(srcs).tobytes() and np.array_equal(m1, a[:, srcs]) and np.array_equal(m2, b2[:, pts2])
    ends = srcs[::-1]
    h1, p1 = api.geodesic_paths(g, srcs, ends)
    hx, px = api.geodesic_paths(g2, pts2, pts2[::-1])
    h2, p2 = api.geodesic_paths(g, srcs, ends)
    assert h1.tobytes() == h2.tobytes()
    for u, v in zip(p1, p2):
        assert (u is None and v is None) or u.tobytes() == v.tobytes()
    w_h, w_p = G.paths(free2, dims2, pts2, pts2[::-1])
    assert np.array_equal(hx, w_h) and all(np.array_equal(u, v) for u, v in zip(px, w_p))
    g2.close()
    other.close()
    g.close()


# ------------------------------------------------------------------ the example
@pytest.mark.parametrize("flags", [["--geodesic"], ["--exact-paths", "--shortcut"]], ids=lambda f: "+".join(f))
def test_plan_batch_flags(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", "--generations", "60"] + flags,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["all_reached"] and out["trajectory_samples"] > 0
    if "--geodesic" in flags:
        q = out["geodesic"]
        assert q["unreachable_pairs"] == [] and q["reachable_pairs"] == 28 and q["searches_at_optimum"] <= 28
        assert q["ratio_mean"] >= 1.0 and q["ratio_max"] >= q["ratio_mean"] and q["left_at_inf"] == []
    else:
        assert out["exact_paths"] and out["lattice_length_total"] >= out["shortened_length_total"]
