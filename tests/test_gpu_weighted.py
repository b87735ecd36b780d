"""GPU tests of the clearance-weighted shortest paths (wa_grid_clearance_costs, wa_grid_weighted_fields / _matrix / _paths) through the
C ABI against the restatement of tests/weighted_ref.py (which follows include/weldacs.h's definitions), scipy's Dijkstra and, where
the fields are too large for either, the local conditions that only the exact field satisfies.  Distances are integers: every
comparison is an equality, there is no tolerance anywhere in this file."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_ref as CR
import geodesic_ref as G
import limit_ref as R
import weighted_ref as W
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, CAPACITY = 1, 7
BANDS = [1, 4, 9]


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


def random_box(dims, occ, wmax, seed):
    """seeded occupancy with a free voxel enclosed by occupied neighbours at the centre (where the box has room), costs drawn from
    1 .. wmax with wmax present (bytes of occupied voxels: anything, 0 and 255 included); returns (free, cost, sources): the corners,
    the pocket and a few random free voxels"""
    nx, ny, nz = dims
    n = nx * ny * nz
    rs = np.random.RandomState(seed)
    free = (rs.uniform(size=n) >= occ).astype(np.uint8)
    corners = [vid(dims, x, y, z) for x, y, z in ((0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, 0), (0, ny - 1, nz - 1))]
    p = vid(dims, nx // 2, ny // 2, nz // 2)
    free[p] = 1
    for v in G.neighbours(p, dims):
        free[v] = 0
    free[corners] = 1
    cand = np.flatnonzero(free)
    srcs = list(dict.fromkeys(corners + [p] + [int(v) for v in cand[rs.randint(len(cand), size=3)]]))
    cost = rs.randint(1, wmax + 1, size=n).astype(np.uint8)
    cost[cand[rs.randint(len(cand))]] = wmax
    cost[free == 0] = rs.choice(np.array([0, 1, 9, 255], np.uint8), size=int((free == 0).sum()))
    return free, cost, srcs


# ------------------------------------------------------------------ 1. fields on random boxes whose x size covers word edges, every W
BOXES = [((1, 1, 1), 0.0, 3), ((63, 1, 1), 0.1, 2), ((64, 1, 1), 0.0, 8), ((65, 1, 1), 0.1, 5), ((129, 1, 1), 0.0, 7), ((1, 7, 5), 0.1, 4),
         ((63, 5, 4), 0.3, 1), ((64, 6, 5), 0.45, 2), ((65, 5, 3), 0.45, 3), ((65, 1, 7), 0.3, 4), ((127, 4, 6), 0.45, 5),
         ((129, 3, 3), 0.3, 6), ((130, 7, 4), 0.45, 7), ((128, 5, 4), 0.2, 8), ((1, 1, 9), 0.3, 6), ((66, 9, 8), 0.0, 8)]


@pytest.mark.parametrize("dims,occ,wmax", BOXES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fields_on_random_boxes(ctx, dims, occ, wmax):
    free, cost, srcs = random_box(dims, occ, wmax, seed=dims[0] * 1000 + dims[1] * 10 + dims[2])
    g = grid_of(ctx, free, dims)
    got = g.weighted_fields(cost, srcs)
    want = W.fields(free, cost, dims, srcs)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    if occ >= 0.45 and np.prod(dims) > 500:
        assert (want[0][free != 0] == W.NONE).mean() > 0.02, "the dense boxes are there for their unreachable voxels"
    m = g.weighted_matrix(cost, srcs)
    assert np.array_equal(m, want[:, srcs])
    g.close()


# ------------------------------------------------------------------ 2. all-ones costs: the bytes of the hop-count entry points
def test_all_ones_is_the_geodesic_field(ctx):
    for dims, occ, seed in (((130, 9, 7), 0.3, 1), ((64, 11, 5), 0.45, 2), ((67, 1, 1), 0.0, 3)):
        free, _, srcs = random_box(dims, occ, 1, seed)
        ones = np.ones(free.size, np.uint8)
        g = grid_of(ctx, free, dims)
        assert g.weighted_fields(ones, srcs).tobytes() == g.geodesic_fields(srcs).tobytes()
        assert g.weighted_matrix(ones, srcs).tobytes() == g.geodesic_matrix(srcs).tobytes()
        ends = srcs[::-1]
        d, n, p = api.weighted_paths(g, ones, srcs, ends)
        h, q = api.geodesic_paths(g, srcs, ends)
        assert d.tobytes() == h.tobytes() and np.array_equal(n, np.maximum(h + 1, 0))
        for a, b in zip(p, q):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
        g.close()


# ------------------------------------------------------------------ 3. chunking
def test_results_do_not_depend_on_the_chunking(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a child process) and all in one launch"""
    dims = (70, 9, 6)
    free, cost, srcs = random_box(dims, 0.3, 6, seed=5)
    g = grid_of(ctx, free, dims)
    f, m = g.weighted_fields(cost, srcs), g.weighted_matrix(cost, srcs)
    d, n, p = api.weighted_paths(g, cost, srcs, srcs[::-1])
    g.close()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "import numpy as np, hashlib\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_weighted import random_box, grid_of\n"
             "free, cost, srcs = random_box((70, 9, 6), 0.3, 6, seed=5)\n"
             "c = api.Context(0); g = grid_of(c, free, (70, 9, 6))\n"
             "d, n, p = api.weighted_paths(g, cost, srcs, srcs[::-1])\n"
             "H = lambda b: hashlib.blake2b(b, digest_size=16).hexdigest()\n"
             "print('digest', H(g.weighted_fields(cost, srcs).tobytes()), H(g.weighted_matrix(cost, srcs).tobytes()),"
             " H(d.tobytes() + n.tobytes() + b''.join(b'' if q is None else q.tobytes() for q in p)))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    H = lambda b: hashlib.blake2b(b, digest_size=16).hexdigest()
    assert line[1] == H(f.tobytes()) and line[2] == H(m.tobytes())
    assert line[3] == H(d.tobytes() + n.tobytes() + b"".join(b"" if q is None else q.tobytes() for q in p))


# ------------------------------------------------------------------ 4. the matrix
def test_matrix_against_fields_and_the_restatement(ctx):
    dims = (97, 12, 10)
    free, cost, srcs = random_box(dims, 0.38, 8, seed=31)
    rs = np.random.RandomState(1)
    cand = np.flatnonzero(free)
    pts = np.array(srcs + [int(v) for v in cand[rs.randint(len(cand), size=12)]], np.int64)
    g = grid_of(ctx, free, dims)
    m = g.weighted_matrix(cost, pts)
    f = g.weighted_fields(cost, pts)
    g.close()
    assert np.array_equal(m, f[:, pts]), "fields and matrix are two routes to the same numbers"
    assert np.array_equal(m, W.matrix(free, cost, dims, pts))
    assert (m < 0).sum() >= 2 * (len(pts) - 1), "the pocket is cut off from every other point"
    c = cost[pts].astype(np.int64)
    reach = m >= 0
    assert np.array_equal(reach, reach.T) and (np.diag(m) == 0).all()
    assert np.array_equal((m - m.T)[reach], (c[None, :] - c[:, None])[reach]), "dist(s, e) - dist(e, s) = cost[e] - cost[s]"
    assert (m != m.T).any()


# ------------------------------------------------------------------ 5. paths
def _raw_paths(ctx, g, cost, starts, ends, off, ids, dist, lens):
    return ctx.lib.wa_grid_weighted_paths(g.h, cost.ctypes.data, starts.ctypes.data, ends.ctypes.data, len(starts), off.ctypes.data,
                                          ids.ctypes.data, dist.ctypes.data, lens.ctypes.data)


def test_paths_against_the_restatement(ctx):
    dims = (67, 11, 9)
    free, cost, _ = random_box(dims, 0.3, 8, seed=77)
    pocket = vid(dims, dims[0] // 2, dims[1] // 2, dims[2] // 2)
    rs = np.random.RandomState(4)
    cand = np.flatnonzero(free)
    reach = np.flatnonzero(W.field(free, cost, dims, 0) >= 0)
    s_pool = [0] + [int(v) for v in reach[rs.randint(len(reach), size=5)]]
    starts = [s_pool[k] for k in rs.randint(len(s_pool), size=40)]           # repeated starts, in no order
    ends = [int(v) for v in cand[rs.randint(len(cand), size=40)]]
    starts[7], ends[7] = s_pool[2], s_pool[2]                                # start == end
    starts[20], ends[20] = s_pool[1], pocket                                 # unreachable, in the middle of the batch
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    g = grid_of(ctx, free, dims)
    w_dist, w_len, w_paths = W.paths(free, cost, dims, starts, ends)
    w_hops = G.paths(free, dims, starts, ends)[0]
    assert w_dist[20] == W.NONE and w_len[20] == 0 and w_dist[7] == 0 and w_len[7] == 1 and (w_len > 20).sum() > 5
    assert (w_len - 1 > w_hops)[w_hops >= 0].sum() > 3, "the case must hold paths that take more steps than the fewest"
    dist, lens, paths = api.weighted_paths(g, cost, starts, ends)
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    for k in range(40):
        if w_dist[k] < 0:
            assert paths[k] is None
            continue
        assert np.array_equal(paths[k], w_paths[k]), k
        W.check_path(free, dims, paths[k], int(starts[k]), int(ends[k]))     # independent of the restatement's walk back
        assert W.path_cost(cost, paths[k]) == dist[k]
    # the raw call: ranges with slack, a sentinel everywhere, nothing written behind a path or into the unreachable pair's range
    SENT = -77
    cap = w_len.astype(np.int64) + 3
    off = np.concatenate([[5], 5 + np.cumsum(cap)]).astype(np.int64)
    ids = np.full(int(off[-1]) + 4, SENT, np.int64)
    d2, l2 = np.full(40, SENT, np.int32), np.full(40, SENT, np.int32)
    assert _raw_paths(ctx, g, cost, starts, ends, off, ids, d2, l2) == 0
    assert np.array_equal(d2, w_dist) and np.array_equal(l2, w_len)
    assert (ids[:5] == SENT).all() and (ids[off[-1]:] == SENT).all()
    for k in range(40):
        L = int(w_len[k])
        if L:
            assert np.array_equal(ids[off[k]:off[k] + L], w_paths[k])
        assert (ids[off[k] + L:off[k + 1]] == SENT).all(), k
    # the capacity round trip: one reachable pair one id short
    k_short = int(np.argmax(w_len))
    cap2 = w_len.astype(np.int64)
    cap2[k_short] -= 1
    off2 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids2 = np.full(int(off2[-1]) + 1, SENT, np.int64)
    d3, l3 = np.full(40, SENT, np.int32), np.full(40, SENT, np.int32)
    assert _raw_paths(ctx, g, cost, starts, ends, off2, ids2, d3, l3) == CAPACITY
    assert np.array_equal(d3, w_dist) and np.array_equal(l3, w_len), "dist_out and len_out are filled for every pair, also on WA_ERR_CAPACITY"
    assert (ids2[off2[k_short]:off2[k_short + 1]] == SENT).all(), "nothing is written for the pair that does not fit"
    for k in range(40):
        if k != k_short and w_dist[k] >= 0:
            assert np.array_equal(ids2[off2[k]:off2[k + 1]], w_paths[k])
    cap2[k_short] += 1                                                       # sized from len_out: the second call succeeds
    off3 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids3 = np.full(int(off3[-1]) + 1, SENT, np.int64)
    assert _raw_paths(ctx, g, cost, starts, ends, off3, ids3, d3, l3) == 0
    assert np.array_equal(ids3[off3[k_short]:off3[k_short + 1]], w_paths[k_short])
    g.close()


def test_hand_cases_and_the_tie(ctx):
    for name, free, cost, dims, src, want, want_paths in W.hand_cases():
        g = grid_of(ctx, free, dims)
        f = g.weighted_fields(cost, [src])[0]
        for v, k in want.items():
            assert f[v] == k, (name, v)
        ends = list(want_paths)
        d, n, p = api.weighted_paths(g, cost, [src] * len(ends), ends)
        for e, q, dd, nn in zip(ends, p, d, n):
            assert q.tolist() == want_paths[e] and dd == want[e] and nn == len(want_paths[e]), (name, e)
        g.close()
    free, cost, dims, s, e, want = W.tie_case()
    g = grid_of(ctx, free, dims)
    d, n, p = api.weighted_paths(g, cost, [s, s], [e, s])
    assert d.tolist() == [4, 0] and n.tolist() == [5, 1] and p[0].tolist() == want and p[1].tolist() == [0]
    g.close()


# ------------------------------------------------------------------ 6. distances beyond 16 bits
def test_serpentine_with_alternating_costs_beyond_16_bits(ctx):
    """600 x 66 x 1, a wall on every second row with its gap at alternating ends: 19 833 free voxels in one line.  The cost alternates
    1, 8 along the corridor (voxel number k from the start costs 8 when k is odd), so the voxel k steps away is at 4.5 k rounded down
    to what the sum gives: the far end at 89 244, far beyond 65 535.  One voxel per 4.5 levels; the path is the whole line."""
    nx, ny = 600, 66
    dims = (nx, ny, 1)
    free = G.serpentine(nx, ny)
    hops = G.queue_field(free, dims, 0)
    n_free = int(free.sum())
    assert n_free == 33 * nx + 33 and hops.max() == n_free - 1
    cost = np.where(hops % 2 == 1, 8, 1).astype(np.uint8)
    cost[free == 0] = 0
    line = np.argsort(np.where(hops >= 0, hops, 1 << 30), kind="stable")[:n_free]
    want = np.full(free.size, W.NONE, np.int32)
    want[line] = np.concatenate([[0], np.cumsum(cost[line][1:].astype(np.int64))])
    far = int(line[-1])
    assert want[far] == 89244 and want.max() > 65535
    g = grid_of(ctx, free, dims)
    f = g.weighted_fields(cost, [0])[0]
    assert np.array_equal(f, want)
    mid = int(line[7001])
    m = g.weighted_matrix(cost, [0, far, mid])
    assert m[0, 1] == want[far] and m[0, 2] == want[mid] and m[1, 0] == want[far] + int(cost[0]) - int(cost[far])
    assert m[2, 1] == want[far] - want[mid]
    d, n, p = api.weighted_paths(g, cost, [0, far], [far, mid])
    assert d.tolist() == [int(m[0, 1]), int(m[1, 2])] and n.tolist() == [n_free, n_free - 7001]
    assert np.array_equal(p[0], line) and np.array_equal(p[1], line[7001:][::-1])
    g.close()


def test_baffles_with_alternating_costs_beyond_16_bits(ctx):
    """1400 x 14 x 14 with a wall at every second x, their gaps at alternating corners: about 18 000 hops from end to end.  Costs 1 and
    8 alternate with x + y + z, that is along any lattice path: the far corner lies beyond 65 535.  Against scipy's Dijkstra."""
    dims = (1400, 14, 14)
    free = G.baffles(*dims, every=2)
    n = int(np.prod(dims))
    v = np.arange(n)
    parity = (v % dims[0] + (v // dims[0]) % dims[1] + v // (dims[0] * dims[1])) % 2
    cost = np.where(parity == 1, 8, 1).astype(np.uint8)
    pts = [0, n - 1]
    want = W.scipy_fields(free, cost, dims, pts)
    assert want[0][n - 1] > 65535
    g = grid_of(ctx, free, dims)
    assert np.array_equal(g.weighted_fields(cost, pts), want)
    assert np.array_equal(g.weighted_matrix(cost, pts), want[:, pts])
    d, ln, p = api.weighted_paths(g, cost, [0], [n - 1])
    W.check_path(free, dims, p[0], 0, n - 1)
    assert d[0] == want[0][n - 1] == W.path_cost(cost, p[0]) and ln[0] == len(p[0])
    g.close()


# ------------------------------------------------------------------ 7. a property that needs no reference
def test_weighted_paths_cost_no_more_and_step_no_less_than_the_hop_optimal_ones(ctx):
    n, P = 96, 16
    free, cx, cy, cz, prec, wall = synth.synth_grid(n)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, P, seed=7)
    cost = g.clearance_costs(BANDS)
    assert set(np.unique(cost).tolist()) == {0, 1, 2, 3, 4} and np.array_equal(cost == 0, free == 0)
    ii, jj = np.triu_indices(P, 1)
    starts, ends = np.concatenate([pts[ii], pts[jj]]), np.concatenate([pts[jj], pts[ii]])     # both directions of all 120 pairs
    dist, lens, paths = api.weighted_paths(g, cost, starts, ends)
    hops, hpaths = api.geodesic_paths(g, starts, ends)
    assert (hops >= 0).all() and (dist >= 0).all()
    dims = (n, n, n)
    cheaper = longer = 0
    for k in range(len(starts)):
        W.check_path(free, dims, paths[k], int(starts[k]), int(ends[k]))
        assert lens[k] == len(paths[k]) >= hops[k] + 1
        assert W.path_cost(cost, paths[k]) == dist[k] <= W.path_cost(cost, hpaths[k])
        cheaper += dist[k] < W.path_cost(cost, hpaths[k])
        longer += lens[k] > hops[k] + 1
    print("weighted paths cheaper than the hop-optimal one: %d of %d, with more steps: %d" % (cheaper, len(starts), longer))
    m = g.weighted_matrix(cost, pts)
    assert np.array_equal(m[ii, jj], dist[:len(ii)]) and np.array_equal(m[jj, ii], dist[len(ii):])
    g.close()


# ------------------------------------------------------------------ 8. the benchmark grids
def test_clearance_costs_against_the_restatement(ctx):
    for dims, occ in (((37, 9, 6), 0.05), ((64, 5, 5), 0.02), ((130, 4, 3), 0.1), ((5, 4, 3), 0.0)):
        n = int(np.prod(dims))
        free = (np.random.RandomState(n).uniform(size=n) >= occ).astype(np.uint8)
        g = grid_of(ctx, free, dims)
        d2 = CR.edt_separable(free, *dims)
        assert np.array_equal(g.distance_field(), d2)
        for thr in (BANDS, [9, 1, 4], [], [0], [2, 2, 5], [1, 2, 3, 4, 5, 6, 7], [W.D2_NONE - 1]):
            got = g.clearance_costs(thr)
            assert got.dtype == np.uint8 and np.array_equal(got, W.clearance_costs(free, d2, thr)), (dims, thr)
        if occ == 0.0:
            assert (g.clearance_costs(BANDS) == 1).all(), "no obstacle: WA_D2_NONE everywhere, cost 1 everywhere"
        g.close()


def test_fields_synth_128_against_scipy(ctx):
    n = 128
    free = synth.synth_grid(n)[0]
    pts = synth.synth_weld_points(free, n, 64)
    g = grid_of(ctx, free, (n, n, n))
    cost = g.clearance_costs(BANDS)
    assert np.array_equal(cost, W.clearance_costs(free, CR.edt_separable(free, n, n, n), BANDS))
    which = [0, 21, 42, 63]
    f = g.weighted_fields(cost, pts[which])
    m = g.weighted_matrix(cost, pts)
    g.close()
    assert np.array_equal(f, W.scipy_fields(free, cost, (n, n, n), pts[which]))
    assert np.array_equal(m[which], f[:, pts])
    c = cost[pts].astype(np.int64)
    assert (m >= 0).all() and np.array_equal(m - m.T, c[None, :] - c[:, None])


def test_c5_full_size(ctx):
    """256^3 synth_grid, C5's 64 weld points, clearance bands 1, 4, 9: two whole fields proven by the local conditions, the matrix rows of
    those sources equal to the fields at the points, the whole matrix held to the asymmetry identity"""
    n = 256
    dims = (n, n, n)
    free = synth.synth_grid(n)[0]
    pts = synth.synth_weld_points(free, n, 64)
    g = grid_of(ctx, free, dims)
    cost = g.clearance_costs(BANDS)
    which = [5, 58]
    f = g.weighted_fields(cost, pts[which])
    m = g.weighted_matrix(cost, pts)
    g.close()
    for k, i in enumerate(which):
        assert W.locally_exact(f[k], free, cost, dims, int(pts[i])), i
    assert np.array_equal(m[which], f[:, pts])
    c = cost[pts].astype(np.int64)
    assert (m >= 0).all() and (np.diag(m) == 0).all() and np.array_equal(m - m.T, c[None, :] - c[:, None])


def test_one_source_at_the_solvers_limit(ctx):
    """2^27 voxels (512^3, limit_ref.box_free at 10 %), one source, random costs 1 .. 8.  Which voxels are reachable:
    scipy.ndimage.label.  The distances: exact at EVERY voxel by the local conditions of weighted_ref.locally_exact
    (tests/test_weighted_rules.py checks the checker)."""
    from scipy import ndimage
    dims = (512, 512, 512)
    src = vid(dims, 17, 300, 255)
    free = R.box_free(dims, 11, 0.10, [src])
    cost = np.empty(free.size, np.uint8)
    for z in range(512):
        cost[z << 18:(z + 1) << 18] = np.random.RandomState(5000 + z).randint(1, 9, size=1 << 18)
    g = grid_of(ctx, free, dims)
    d = g.weighted_fields(cost, [src])[0]
    g.close()
    lab, _ = ndimage.label(free.reshape(512, 512, 512) != 0)
    lab = lab.reshape(-1)
    assert np.array_equal(d >= 0, lab == lab[src])
    del lab
    assert W.locally_exact(d, free, cost, dims, src)


# ------------------------------------------------------------------ 9. arguments
def test_arguments(ctx):
    dims = (9, 4, 3)
    free = np.ones(108, np.uint8)
    free[50] = 0
    g = grid_of(ctx, free, dims)
    lib = ctx.lib
    SENT = -77
    out = np.full(4 * 108, SENT, np.int32)
    lens = np.full(8, SENT, np.int32)
    ids_out = np.full(64, SENT, np.int64)
    cost_out = np.full(108, 0x55, np.uint8)
    off = np.array([0, 30, 60], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ok_ids = i64(0, 107)
    ok_cost = np.full(108, 2, np.uint8)
    ok_cost[50] = 0                                                            # (an occupied voxel's byte is ignored)
    P = lambda a: a.ctypes.data

    def untouched():
        return (out == SENT).all() and (ids_out == SENT).all() and (lens == SENT).all() and (cost_out == 0x55).all()

    def both_paths(cost, a, b, cnt, off_=off):
        return (lib.wa_grid_weighted_paths(g.h, cost, a, b, cnt, P(off_), P(ids_out), P(out), P(lens)),
                lib.wa_grid_weighted_paths(g.h, cost, b, a, cnt, P(off_), P(ids_out), P(out), P(lens)))

    def all_three(cost, a, b, cnt):
        return (lib.wa_grid_weighted_fields(g.h, cost, a, cnt, P(out)), lib.wa_grid_weighted_matrix(g.h, cost, a, cnt, P(out))) + both_paths(cost, a, b, cnt)

    for bad in (i64(0, 50), i64(0, 108), i64(-1, 0), i64(0, 1 << 40)):       # occupied, outside (above, below, far above)
        assert all_three(P(ok_cost), P(bad), P(ok_ids), 2) == (ARG,) * 4 and untouched()
    # costs: 0 on a free voxel, above WA_COST_MAX
    for v, c in ((3, 0), (107, 9), (0, 255)):
        bad_cost = ok_cost.copy()
        bad_cost[v] = c
        assert all_three(P(bad_cost), P(ok_ids), P(ok_ids), 2) == (ARG,) * 4 and untouched()
        assert b"cost" in lib.wa_last_error(ctx.h)
    # negative counts, NULL arrays (also with a count of 0), NULL outputs, decreasing offsets
    assert all_three(P(ok_cost), P(ok_ids), P(ok_ids), -1) == (ARG,) * 4
    for cnt in (0, 2):
        assert all_three(None, P(ok_ids), P(ok_ids), cnt) == (ARG,) * 4
        assert all_three(P(ok_cost), None, None, cnt) == (ARG,) * 4
        assert both_paths(P(ok_cost), P(ok_ids), None, cnt) == (ARG,) * 2
        assert lib.wa_grid_weighted_fields(g.h, P(ok_cost), P(ok_ids), cnt, None) == ARG
        assert lib.wa_grid_weighted_matrix(g.h, P(ok_cost), P(ok_ids), cnt, None) == ARG
        for k in range(4):
            a = [P(off), P(ids_out), P(out), P(lens)]
            a[k] = None
            assert lib.wa_grid_weighted_paths(g.h, P(ok_cost), P(ok_ids), P(ok_ids), cnt, *a) == ARG
    down = np.array([0, 30, 29], np.int64)
    assert both_paths(P(ok_cost), P(ok_ids), P(ok_ids), 2, down) == (ARG,) * 2
    # thresholds
    thr = np.array([1, 4, 9, 16, 25, 36, 49, 64], np.int32)
    assert lib.wa_grid_clearance_costs(g.h, P(thr), 8, P(cost_out)) == ARG, "more than WA_COST_MAX - 1 thresholds"
    assert lib.wa_grid_clearance_costs(g.h, P(thr), -1, P(cost_out)) == ARG
    assert lib.wa_grid_clearance_costs(g.h, None, 0, P(cost_out)) == ARG
    assert lib.wa_grid_clearance_costs(g.h, P(thr), 3, None) == ARG
    for t in (-1, W.D2_NONE):
        assert lib.wa_grid_clearance_costs(g.h, P(np.array([1, t], np.int32)), 2, P(cost_out)) == ARG
    assert untouched()
    # counts of zero with valid pointers succeed and write nothing
    assert all_three(P(ok_cost), P(ok_ids), P(ok_ids), 0) == (0,) * 4 and untouched()
    # and everything still works
    assert lib.wa_grid_clearance_costs(g.h, P(thr), 7, P(cost_out)) == 0 and cost_out[50] == 0 and cost_out[49] == 8
    assert np.array_equal(cost_out, W.clearance_costs(free, CR.edt_brute(free, *dims), thr[:7]))
    assert np.array_equal(g.occupancy(), free)
    assert g.weighted_matrix(ok_cost, ok_ids).tolist() == [[0, 2 * 13], [2 * 13, 0]]
    g.close()


def test_a_grid_whose_distances_might_not_fit_int32_is_refused(ctx):
    """1024 x 1024 x 257, all free, cost 8 everywhere: 8 * (n - 1) = 2^31 + 2^23 - 8 > 2^31 - 1.  Refused before any search starts (a
    search of this grid would take minutes; the call returns in the time of the upload)."""
    dims = (1024, 1024, 257)
    n = int(np.prod(dims))
    assert n > 1 << 28 and 8 * (n - 1) > 2 ** 31 - 1 >= 7 * (n - 1)
    free = np.ones(n, np.uint8)
    g = grid_of(ctx, free, dims)
    del free
    cost = np.full(n, 8, np.uint8)
    SENT = -77
    out, lens, ids_out = np.full(16, SENT, np.int32), np.full(4, SENT, np.int32), np.full(16, SENT, np.int64)
    pts = np.array([0, n - 1], np.int64)
    off = np.array([0, 8, 16], np.int64)
    P = lambda a: a.ctypes.data
    assert ctx.lib.wa_grid_weighted_matrix(g.h, P(cost), P(pts), 2, P(out)) == ARG
    assert b"int32" in ctx.lib.wa_last_error(ctx.h)
    assert ctx.lib.wa_grid_weighted_paths(g.h, P(cost), P(pts), P(pts[::-1].copy()), 2, P(off), P(ids_out), P(out), P(lens)) == ARG
    assert (out == SENT).all() and (lens == SENT).all() and (ids_out == SENT).all()
    g.close()


# ------------------------------------------------------------------ 10. repeatability, two contexts
def test_same_bytes_twice_and_two_contexts(ctx):
    dims = (130, 20, 12)
    free, cost, srcs = random_box(dims, 0.3, 8, seed=9)
    other = api.Context(0)
    dims2 = (65, 9, 9)
    free2 = G.baffles(*dims2)
    cost2 = np.random.RandomState(3).randint(1, 6, size=free2.size).astype(np.uint8)
    g, g2 = grid_of(ctx, free, dims), grid_of(other, free2, dims2)
    pts2 = [0, int(np.prod(dims2)) - 1, 300]
    a = g.weighted_fields(cost, srcs)
    b2 = g2.weighted_fields(cost2, pts2)
    b = g.weighted_fields(cost, srcs)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, W.fields(free, cost, dims, srcs)) and np.array_equal(b2, W.fields(free2, cost2, dims2, pts2))
    m1, m2 = g.weighted_matrix(cost, srcs), g2.weighted_matrix(cost2, pts2)
    assert m1.tobytes() == g.weighted_matrix(cost, srcs).tobytes() and np.array_equal(m1, a[:, srcs]) and np.array_equal(m2, b2[:, pts2])
    ends = srcs[::-1]
    d1, n1, p1 = api.weighted_paths(g, cost, srcs, ends)
    dx, nx_, px = api.weighted_paths(g2, cost2, pts2, pts2[::-1])
    d2, n2, p2 = api.weighted_paths(g, cost, srcs, ends)
    assert d1.tobytes() == d2.tobytes() and n1.tobytes() == n2.tobytes()
    for u, v in zip(p1, p2):
        assert (u is None and v is None) or u.tobytes() == v.tobytes()
    w_d, w_n, w_p = W.paths(free2, cost2, dims2, pts2, pts2[::-1])
    assert np.array_equal(dx, w_d) and np.array_equal(nx_, w_n) and all(np.array_equal(u, v) for u, v in zip(px, w_p))
    # a second cost array on the same grid right after: nothing of the first is kept
    ones = np.ones(free.size, np.uint8)
    assert g.weighted_fields(ones, srcs).tobytes() == g.geodesic_fields(srcs).tobytes()
    assert g.weighted_fields(cost, srcs).tobytes() == a.tobytes()
    g2.close()
    other.close()
    g.close()


# ------------------------------------------------------------------ the example
def test_plan_batch_safe_paths():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", "--safe-paths", "3", "--shortcut"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["all_reached"] and out["trajectory_samples"] > 0 and out["lattice_length_total"] >= out["shortened_length_total"]
    q = out["safe_paths"]
    for key in ("t_costs_s", "t_paths_s", "bands", "nodes_total", "extra_steps_total", "nodes_within_bands", "nodes_within_bands_hop_optimal",
                "n_hit", "n_hit_hop_optimal"):
        assert key in q, key
    assert q["bands"] == [1, 4, 9] and q["extra_steps_total"] >= 0 and q["nodes_total"] >= 28 * 2
    assert q["extra_steps_total"] % 2 == 0, "the lattice is bipartite: every path exceeds the hop count by an even number of steps"
