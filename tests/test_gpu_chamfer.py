"""GPU tests of the 26-neighbour chamfer fields (wa_grid_chamfer_fields / _matrix / _paths) through the C ABI against the restatement of
tests/chamfer_ref.py (which follows include/weldacs.h's definitions), the identities the header states and, where a field is too large
for a Python heap, the local conditions that only the exact field satisfies.  Distances are integers: every comparison is an equality,
there is no tolerance anywhere in this file."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chamfer_ref as C
import geodesic_ref as G
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, CAPACITY = 1, 7
STEPS = [(3, 4, 5), (1, 1, 1), (1, 2, 3), (5, 7, 9), (2, 3, 16), (16, 1, 7)]


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


def random_box(dims, occ, seed):
    """seeded occupancy with a free voxel enclosed by its six occupied face neighbours at the centre (where the box has room; the box rule
    cuts it off although diagonal neighbours may be free); returns (free, sources): the corners, the pocket and a few random free voxels"""
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
    return free, srcs


# ------------------------------------------------------------------ 1. word edges and small boxes, every step triple
BOXES = [((1, 1, 1), 0.0), ((63, 1, 1), 0.1), ((64, 2, 1), 0.1), ((65, 3, 1), 0.2), ((129, 2, 2), 0.2), ((1, 7, 5), 0.2), ((63, 5, 4), 0.3),
         ((64, 6, 5), 0.3), ((65, 5, 3), 0.3), ((65, 1, 7), 0.2), ((127, 4, 6), 0.3), ((129, 3, 3), 0.3), ((128, 5, 4), 0.2), ((66, 9, 8), 0.15)]


def box_case(k):
    """(dims, step, free, sources, starts, ends) of box k.  The pairs: every source to the source opposite in the list, and from each of
    the first three sources to the voxel farthest from it (by the restatement), so that long reachable pairs exist in every box."""
    dims, occ = BOXES[k]
    step = STEPS[k % len(STEPS)]
    free, srcs = random_box(dims, occ, seed=dims[0] * 1000 + dims[1] * 10 + dims[2])
    want = C.fields(free, step, dims, srcs)
    starts, ends = list(srcs), list(srcs[::-1])
    for i in range(min(3, len(srcs))):
        starts.append(srcs[i])
        ends.append(int(np.argmax(want[i])))
    return dims, step, free, srcs, want, np.array(starts, np.int64), np.array(ends, np.int64)


@pytest.mark.parametrize("k", range(len(BOXES)), ids=["x".join(map(str, b[0])) for b in BOXES])
def test_fields_matrix_and_paths_on_random_boxes(ctx, k):
    dims, step, free, srcs, want, starts, ends = box_case(k)
    w_dist, w_len, w_paths = C.paths(free, step, dims, starts, ends)
    by_class = sum((C.moves_by_class(dims, p) for p in w_paths if p is not None), np.zeros(3, np.int64))
    if dims[1] * dims[2] > 1:
        # the case exercises the rule, by the restatement alone
        assert C.forbidden_moves(free, dims) >= 1, "a move between two free voxels that the box rule forbids"
        if step == (1, 2, 3):
            assert by_class[1] == 0 and by_class[2] == 0, "with {1, 2, 3} the face-first order never takes a diagonal (header identity)"
        else:
            assert by_class[1] >= 1, "a returned path uses an edge move"
    g = grid_of(ctx, free, dims)
    got = g.chamfer_fields(step, srcs)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(g.chamfer_matrix(step, srcs), want[:, srcs])
    dist, lens, paths = api.chamfer_paths(g, step, starts, ends)
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    for i, (p, q) in enumerate(zip(paths, w_paths)):
        assert (p is None and q is None) or np.array_equal(p, q), i
    g.close()


def test_the_boxes_hold_corner_moves():
    """over the boxes above, by the restatement alone (nothing here depends on the order the tests ran in)"""
    total = 0
    for k in (7, 11, 13):
        dims, step, free, srcs, want, starts, ends = box_case(k)
        total += sum(int(C.moves_by_class(dims, p)[2]) for p in C.paths(free, step, dims, starts, ends)[2] if p is not None)
    assert total >= 1, "a returned path uses a corner move"


# ------------------------------------------------------------------ 2. step = {1, 2, 3}: the bytes of the hop-count entry points
def test_1_2_3_is_the_geodesic_field(ctx):
    for dims, occ, seed in (((130, 9, 7), 0.3, 1), ((64, 11, 5), 0.25, 2), ((67, 1, 1), 0.0, 3)):
        free, srcs = random_box(dims, occ, seed)
        g = grid_of(ctx, free, dims)
        assert g.chamfer_fields((1, 2, 3), srcs).tobytes() == g.geodesic_fields(srcs).tobytes()
        assert g.chamfer_matrix((1, 2, 3), srcs).tobytes() == g.geodesic_matrix(srcs).tobytes()
        ends = srcs[::-1]
        d, n, p = api.chamfer_paths(g, (1, 2, 3), srcs, ends)
        h, q = api.geodesic_paths(g, srcs, ends)
        assert d.tobytes() == h.tobytes() and np.array_equal(n, np.maximum(h + 1, 0))
        assert (h > 5).any()
        for a, b in zip(p, q):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
        g.close()


# ------------------------------------------------------------------ 3. closed forms without obstacles
def test_closed_forms(ctx):
    dims = (9, 7, 5)
    free = np.ones(int(np.prod(dims)), np.uint8)
    g = grid_of(ctx, free, dims)
    srcs = [0, 157, 314, vid(dims, 8, 0, 4)]
    for step in ((1, 1, 1), (3, 4, 5)):
        got = g.chamfer_fields(step, srcs)
        for s, f in zip(srcs, got):
            assert np.array_equal(f, C.closed_form(step, dims, s)), (step, s)
    g.close()


# ------------------------------------------------------------------ 4. the matrix
def test_matrix_symmetry_rows_and_pockets(ctx):
    dims = (97, 12, 10)
    free, srcs = random_box(dims, 0.25, seed=31)          # its pocket: only the six face neighbours occupied
    face_pocket = srcs[4]
    assert face_pocket == vid(dims, 48, 6, 5)
    # a second pocket with all 26 neighbours occupied
    full_pocket = vid(dims, 20, 4, 4)
    for dx, dy, dz in C.OFFSETS:
        free[full_pocket + dx + dims[0] * (dy + dims[1] * dz)] = 0
    free[full_pocket] = 1
    assert free[srcs].all(), "no source lies beside the second pocket"
    nb26 = [face_pocket + dx + dims[0] * (dy + dims[1] * dz) for dx, dy, dz in C.OFFSETS[6:]]
    assert free[nb26].sum() > 0, "the face pocket has free diagonal neighbours: only the box rule cuts it off"
    rs = np.random.RandomState(1)
    cand = np.flatnonzero(free)
    pts = np.array(list(dict.fromkeys(srcs + [full_pocket] + [int(v) for v in cand[rs.randint(len(cand), size=10)]])), np.int64)
    step = (3, 4, 5)
    g = grid_of(ctx, free, dims)
    m = g.chamfer_matrix(step, pts)
    f = g.chamfer_fields(step, pts)
    g.close()
    assert np.array_equal(m, m.T) and (np.diag(m) == 0).all()
    assert np.array_equal(m, f[:, pts]), "fields and matrix are two routes to the same numbers"
    assert np.array_equal(m, C.matrix(free, step, dims, pts))
    for pocket in (face_pocket, full_pocket):
        i = int(np.flatnonzero(pts == pocket)[0])
        others = np.arange(len(pts)) != i
        assert (m[i, others] == C.NONE).all() and (m[others, i] == C.NONE).all(), "an enclosed pocket: WA_DIST_NONE both ways"
        assert (f[i] >= 0).sum() == 1
    assert (m >= 0).sum() > len(pts) ** 2 // 2


# ------------------------------------------------------------------ 5. paths
def _raw_paths(ctx, g, step, starts, ends, off, ids, dist, lens):
    step = np.asarray(step, np.int32)
    return ctx.lib.wa_grid_chamfer_paths(g.h, step.ctypes.data, starts.ctypes.data, ends.ctypes.data, len(starts), off.ctypes.data,
                                         ids.ctypes.data, dist.ctypes.data, lens.ctypes.data)


def test_paths_protocol_and_clearance(ctx):
    dims = (67, 11, 9)
    step = (3, 4, 5)
    free, _ = random_box(dims, 0.2, seed=77)
    pocket = vid(dims, dims[0] // 2, dims[1] // 2, dims[2] // 2)
    rs = np.random.RandomState(4)
    moves = C._flat_moves(free, dims)
    reach = np.flatnonzero(C.field(free, step, dims, 0, moves) >= 0)
    s_pool = [0] + [int(v) for v in reach[rs.randint(len(reach), size=5)]]
    cand = np.flatnonzero(free)
    starts = [s_pool[k] for k in rs.randint(len(s_pool), size=40)]           # repeated starts, in no order
    ends = [int(v) for v in cand[rs.randint(len(cand), size=40)]]
    starts[7], ends[7] = s_pool[2], s_pool[2]                                # start == end
    starts[20], ends[20] = s_pool[1], pocket                                 # unreachable, in the middle of the batch
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    w_dist, w_len, w_paths = C.paths(free, step, dims, starts, ends)
    assert w_dist[20] == C.NONE and w_len[20] == 0 and w_dist[7] == 0 and w_len[7] == 1 and (w_len > 15).sum() > 5
    g = grid_of(ctx, free, dims)
    dist, lens, paths = api.chamfer_paths(g, step, starts, ends)
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    by_class = np.zeros(3, np.int64)
    for k in range(40):
        if w_dist[k] < 0:
            assert paths[k] is None
            continue
        assert np.array_equal(paths[k], w_paths[k]), k
        C.check_path(free, dims, paths[k], int(starts[k]), int(ends[k]))     # 26-steps and the box rule, independent of the walk back
        assert C.path_cost(step, dims, paths[k]) == dist[k]
        by_class += C.moves_by_class(dims, paths[k])
    assert (by_class > 0).all(), "face, edge and corner moves all occur"
    # a path has no hit in wa_traj_clearance: unit-spaced grid, nodes map to themselves
    for k in np.argsort(-w_len)[:8]:
        p = paths[int(k)]
        xyz = np.stack([p % dims[0], (p // dims[0]) % dims[1], p // (dims[0] * dims[1])], axis=1).astype(np.float32)
        t = api.Trajectory.from_points(ctx, xyz)
        ids, _, hit, summary = t.clearance(g)
        assert np.array_equal(ids, p) and summary["n_hit"] == 0 and summary["n_outside"] == 0 and not hit.any()
        t.close()
    # the raw call: ranges with slack, a sentinel everywhere, nothing written behind a path or into the unreachable pair's range
    SENT = -77
    cap = w_len.astype(np.int64) + 3
    off = np.concatenate([[5], 5 + np.cumsum(cap)]).astype(np.int64)
    ids = np.full(int(off[-1]) + 4, SENT, np.int64)
    d2, l2 = np.full(40, SENT, np.int32), np.full(40, SENT, np.int32)
    assert _raw_paths(ctx, g, step, starts, ends, off, ids, d2, l2) == 0
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
    assert _raw_paths(ctx, g, step, starts, ends, off2, ids2, d3, l3) == CAPACITY
    assert np.array_equal(d3, w_dist) and np.array_equal(l3, w_len), "dist_out and len_out are filled for every pair, also on WA_ERR_CAPACITY"
    assert (ids2[off2[k_short]:off2[k_short + 1]] == SENT).all(), "nothing is written for the pair that does not fit"
    for k in range(40):
        if k != k_short and w_dist[k] >= 0:
            assert np.array_equal(ids2[off2[k]:off2[k + 1]], w_paths[k])
    cap2[k_short] += 1                                                       # sized from len_out: the second call succeeds
    off3 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids3 = np.full(int(off3[-1]) + 1, SENT, np.int64)
    assert _raw_paths(ctx, g, step, starts, ends, off3, ids3, d3, l3) == 0
    assert np.array_equal(ids3[off3[k_short]:off3[k_short + 1]], w_paths[k_short])
    g.close()


def test_hand_cases(ctx):
    for name, free, step, dims, src, want, want_paths in C.hand_cases():
        g = grid_of(ctx, free, dims)
        f = g.chamfer_fields(step, [src])[0]
        for v, k in want.items():
            assert f[v] == k, (name, v)
        ends = list(want_paths)
        d, n, p = api.chamfer_paths(g, step, [src] * len(ends), ends)
        for e, q, dd, nn in zip(ends, p, d, n):
            assert q.tolist() == want_paths[e] and dd == want[e] and nn == len(want_paths[e]), (name, e)
        g.close()


# ------------------------------------------------------------------ 6. distances beyond 16 bits
def test_serpentine_beyond_16_bits(ctx):
    """600 x 66 x 1, a wall on every second row with its gap at alternating ends: 19 833 free voxels in one line.  Every diagonal at a
    turn spans an occupied voxel, so with {4, 5, 6} dist = 4 * hops: 79 328 at the far end, beyond 65 535."""
    nx, ny = 600, 66
    dims = (nx, ny, 1)
    step = (4, 5, 6)
    free = G.serpentine(nx, ny)
    hops = G.queue_field(free, dims, 0)
    n_free = int(free.sum())
    assert n_free == 33 * nx + 33 and hops.max() == n_free - 1
    want = np.where(hops >= 0, 4 * hops, C.NONE).astype(np.int32)
    assert C.locally_exact(want, free, step, dims, 0), "the restatement first: 4 * hops is THE chamfer field of the serpentine"
    line = np.argsort(np.where(hops >= 0, hops, 1 << 30), kind="stable")[:n_free]
    far = int(line[-1])
    assert want[far] == 79328 and want.max() > 65535
    g = grid_of(ctx, free, dims)
    f = g.chamfer_fields(step, [0])[0]
    assert np.array_equal(f, want)
    mid = int(line[7001])
    m = g.chamfer_matrix(step, [0, far, mid])
    assert m[0, 1] == want[far] and m[0, 2] == want[mid] and m[2, 1] == want[far] - want[mid] and np.array_equal(m, m.T)
    d, n, p = api.chamfer_paths(g, step, [0, far], [far, mid])
    assert d.tolist() == [int(m[0, 1]), int(m[1, 2])] and n.tolist() == [n_free, n_free - 7001]
    assert np.array_equal(p[0], line) and np.array_equal(p[1], line[7001:][::-1])
    g.close()


# ------------------------------------------------------------------ 7. chunking
def test_results_do_not_depend_on_the_chunking(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a fresh child process) and all in one launch"""
    dims = (70, 9, 6)
    step = (2, 3, 16)
    free, srcs = random_box(dims, 0.2, seed=5)
    g = grid_of(ctx, free, dims)
    f, m = g.chamfer_fields(step, srcs), g.chamfer_matrix(step, srcs)
    d, n, p = api.chamfer_paths(g, step, srcs, srcs[::-1])
    g.close()
    assert (d > 0).any()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "import numpy as np, hashlib\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_chamfer import random_box, grid_of\n"
             "free, srcs = random_box((70, 9, 6), 0.2, seed=5)\n"
             "c = api.Context(0); g = grid_of(c, free, (70, 9, 6))\n"
             "d, n, p = api.chamfer_paths(g, (2, 3, 16), srcs, srcs[::-1])\n"
             "H = lambda b: hashlib.blake2b(b, digest_size=16).hexdigest()\n"
             "print('digest', H(g.chamfer_fields((2, 3, 16), srcs).tobytes()), H(g.chamfer_matrix((2, 3, 16), srcs).tobytes()),"
             " H(d.tobytes() + n.tobytes() + b''.join(b'' if q is None else q.tobytes() for q in p)))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    H = lambda b: hashlib.blake2b(b, digest_size=16).hexdigest()
    assert line[1] == H(f.tobytes()) and line[2] == H(m.tobytes())
    assert line[3] == H(d.tobytes() + n.tobytes() + b"".join(b"" if q is None else q.tobytes() for q in p))


# ------------------------------------------------------------------ 8. repeatability, two contexts
def test_same_bytes_twice_and_two_contexts(ctx):
    dims = (130, 12, 8)
    step = (5, 7, 9)
    free, srcs = random_box(dims, 0.2, seed=9)
    other = api.Context(0)
    dims2 = (65, 7, 5)
    free2 = G.baffles(*dims2)
    step2 = (16, 1, 7)
    g, g2 = grid_of(ctx, free, dims), grid_of(other, free2, dims2)
    pts2 = [0, int(np.prod(dims2)) - 1, 300]
    a = g.chamfer_fields(step, srcs)
    b2 = g2.chamfer_fields(step2, pts2)
    b = g.chamfer_fields(step, srcs)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, C.fields(free, step, dims, srcs)) and np.array_equal(b2, C.fields(free2, step2, dims2, pts2))
    m1, m2 = g.chamfer_matrix(step, srcs), g2.chamfer_matrix(step2, pts2)
    assert m1.tobytes() == g.chamfer_matrix(step, srcs).tobytes() and np.array_equal(m1, a[:, srcs]) and np.array_equal(m2, b2[:, pts2])
    ends = srcs[::-1]
    d1, n1, p1 = api.chamfer_paths(g, step, srcs, ends)
    dx, nx_, px = api.chamfer_paths(g2, step2, pts2, pts2[::-1])
    d2, n2, p2 = api.chamfer_paths(g, step, srcs, ends)
    assert d1.tobytes() == d2.tobytes() and n1.tobytes() == n2.tobytes()
    for u, v in zip(p1, p2):
        assert (u is None and v is None) or u.tobytes() == v.tobytes()
    w_d, w_n, w_p = C.paths(free2, step2, dims2, pts2, pts2[::-1])
    assert np.array_equal(dx, w_d) and np.array_equal(nx_, w_n) and all(np.array_equal(u, v) for u, v in zip(px, w_p))
    # a different step on the same grid right after: nothing of the first is kept
    assert g.chamfer_fields((1, 2, 3), srcs).tobytes() == g.geodesic_fields(srcs).tobytes()
    assert g.chamfer_fields(step, srcs).tobytes() == a.tobytes()
    g2.close()
    other.close()
    g.close()


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
    off = np.array([0, 30, 60], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ok_ids = i64(0, 107)
    ok_step = np.array([3, 4, 5], np.int32)
    P = lambda a: a.ctypes.data

    def untouched():
        return (out == SENT).all() and (ids_out == SENT).all() and (lens == SENT).all()

    def both_paths(step, a, b, cnt, off_=off):
        return (lib.wa_grid_chamfer_paths(g.h, step, a, b, cnt, P(off_), P(ids_out), P(out), P(lens)),
                lib.wa_grid_chamfer_paths(g.h, step, b, a, cnt, P(off_), P(ids_out), P(out), P(lens)))

    def all_three(step, a, b, cnt):
        return (lib.wa_grid_chamfer_fields(g.h, step, a, cnt, P(out)), lib.wa_grid_chamfer_matrix(g.h, step, a, cnt, P(out))) + both_paths(step, a, b, cnt)

    for bad in (i64(0, 50), i64(0, 108), i64(-1, 0), i64(0, 1 << 40)):       # occupied, outside (above, below, far above)
        assert all_three(P(ok_step), P(bad), P(ok_ids), 2) == (ARG,) * 4 and untouched()
    # steps: 0, above WA_STEP_MAX, negative, in every position
    for k in range(3):
        for v in (0, 17, -1):
            bad_step = ok_step.copy()
            bad_step[k] = v
            assert all_three(P(bad_step), P(ok_ids), P(ok_ids), 2) == (ARG,) * 4 and untouched()
            assert b"step" in lib.wa_last_error(ctx.h)
    # negative counts, NULL arrays (also with a count of 0), NULL outputs, decreasing offsets
    assert all_three(P(ok_step), P(ok_ids), P(ok_ids), -1) == (ARG,) * 4
    for cnt in (0, 2):
        assert all_three(None, P(ok_ids), P(ok_ids), cnt) == (ARG,) * 4
        assert all_three(P(ok_step), None, None, cnt) == (ARG,) * 4
        assert both_paths(P(ok_step), P(ok_ids), None, cnt) == (ARG,) * 2
        assert lib.wa_grid_chamfer_fields(g.h, P(ok_step), P(ok_ids), cnt, None) == ARG
        assert lib.wa_grid_chamfer_matrix(g.h, P(ok_step), P(ok_ids), cnt, None) == ARG
        for k in range(4):
            a = [P(off), P(ids_out), P(out), P(lens)]
            a[k] = None
            assert lib.wa_grid_chamfer_paths(g.h, P(ok_step), P(ok_ids), P(ok_ids), cnt, *a) == ARG
    down = np.array([0, 30, 29], np.int64)
    assert both_paths(P(ok_step), P(ok_ids), P(ok_ids), 2, down) == (ARG,) * 2
    assert untouched()
    # counts of zero with valid pointers succeed and write nothing
    assert all_three(P(ok_step), P(ok_ids), P(ok_ids), 0) == (0,) * 4 and untouched()
    # and everything still works: (8, 3, 2) apart: 3 * 5 + 4 * 1 + 5 * 2
    assert np.array_equal(g.occupancy(), free)
    assert g.chamfer_matrix(ok_step, ok_ids).tolist() == [[0, 29], [29, 0]]
    assert g.chamfer_matrix((16, 16, 16), ok_ids).tolist() == [[0, 128], [128, 0]]
    g.close()


def test_a_grid_whose_distances_might_not_fit_int32_is_refused(ctx):
    """1024 x 1024 x 129, all free, step {16, 16, 16}: 16 * (n - 1) = 2^31 + 2^24 - 16 > 2^31 - 1.  Refused before any search starts (a
    search of this grid would take minutes; the calls return at once)."""
    dims = (1024, 1024, 129)
    n = int(np.prod(dims))
    assert 16 * (n - 1) > 2 ** 31 - 1 >= 15 * (n - 1)
    free = np.ones(n, np.uint8)
    t0 = time.perf_counter()
    g = grid_of(ctx, free, dims)
    t_grid = time.perf_counter() - t0
    del free
    step = np.array([16, 16, 16], np.int32)
    SENT = -77
    out, lens, ids_out = np.full(16, SENT, np.int32), np.full(4, SENT, np.int32), np.full(16, SENT, np.int64)
    pts = np.array([0, n - 1], np.int64)
    off = np.array([0, 8, 16], np.int64)
    P = lambda a: a.ctypes.data
    t0 = time.perf_counter()
    assert ctx.lib.wa_grid_chamfer_matrix(g.h, P(step), P(pts), 2, P(out)) == ARG
    assert b"int32" in ctx.lib.wa_last_error(ctx.h)
    assert ctx.lib.wa_grid_chamfer_fields(g.h, P(step), P(pts), 2, P(out)) == ARG
    assert ctx.lib.wa_grid_chamfer_paths(g.h, P(step), P(pts), P(pts[::-1].copy()), 2, P(off), P(ids_out), P(out), P(lens)) == ARG
    t_calls = time.perf_counter() - t0
    assert b"int32" in ctx.lib.wa_last_error(ctx.h)
    assert (out == SENT).all() and (lens == SENT).all() and (ids_out == SENT).all()
    assert t_calls <= t_grid, "refused in (less than) the time of building the grid: %.3f s against %.3f s" % (t_calls, t_grid)
    # one step less fits
    step[:] = 15
    assert ctx.lib.wa_grid_chamfer_matrix(g.h, P(step), P(pts[:1]), 1, P(out)) == 0 and out[0] == 0
    g.close()


# ------------------------------------------------------------------ 10. mid-size cross-check
def test_synth_96_cross_check(ctx):
    n, P = 96, 16
    step = (3, 4, 5)
    dims = (n, n, n)
    free, cx, cy, cz, prec, wall = synth.synth_grid(n)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, P, seed=7)
    which = [3, 12]
    f = g.chamfer_fields(step, pts[which])
    m = g.chamfer_matrix(step, pts)
    hops = g.geodesic_matrix(pts)
    g.close()
    for k, i in enumerate(which):
        assert C.locally_exact(f[k], free, step, dims, int(pts[i])), i
    assert np.array_equal(m[which], f[:, pts]) and np.array_equal(m, m.T)
    assert (hops >= 0).all() and (m >= 0).all()
    assert (m <= 3 * hops).all(), "face moves alone give 3 * hops"
    cheb = np.stack([C.chebyshev(dims, int(p)).max(axis=0)[pts] for p in pts])
    assert (m >= 3 * cheb).all(), "every move costs at least 3 and advances the Chebyshev distance by at most 1"
    assert (m < 3 * hops).any()


# ------------------------------------------------------------------ the example
def test_plan_batch_diagonal_paths():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", "--diagonal-paths", "--shortcut"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    q = out["diagonal_paths"]
    for key in ("step", "t_matrix_s", "t_paths_s", "nodes_total", "moves_by_class", "length_total", "n_hit", "shortened_length_total_hop_optimal"):
        assert key in q, key
    assert q["step"] == [3, 4, 5] and q["n_hit"] == 0 and len(q["moves_by_class"]) == 3
    assert sum(q["moves_by_class"]) == q["nodes_total"] - 28 and q["moves_by_class"][1] > 0
    assert out["all_reached"] and out["lattice_length_total"] >= out["shortened_length_total"] > 0
