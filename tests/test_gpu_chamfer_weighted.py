"""GPU tests of the penalised 26-neighbour fields (wa_grid_chamfer_weighted_fields / _matrix / _paths) through the C ABI against the
restatement of tests/chamfer_weighted_ref.py (which follows include/weldacs.h's definitions), the three identities the header states, and
the two planners the new one combines.  Distances are integers: every comparison is an equality, there is no tolerance in this file."""
import functools
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chamfer_ref as C
import chamfer_weighted_ref as CW
import clearance_ref as K
import geodesic_ref as G
import weighted_ref as W
from test_gpu_chamfer import BOXES, STEPS, grid_of, random_box, vid
from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, CAPACITY = 1, 7
SENT = -77
P = lambda a: a.ctypes.data


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def clearance_pen(free, dims, gain=3, bands=(1, 4, 9)):
    """gain * (clearance cost - 1) by the restatements; (cost, pen)"""
    d2 = np.asarray(K.edt_separable(free, *dims)).reshape(-1)
    d2 = np.minimum(d2, W.D2_NONE)
    cost = W.clearance_costs(free, d2, bands)
    return cost, np.where(free != 0, gain * (cost.astype(np.int64) - 1), 0).astype(np.uint8)


def pattern(k, free, dims, seed):
    """the four penalty patterns of the box tests; occupied voxels carry 255 in the random ones (their bytes are ignored)"""
    rs = np.random.RandomState(seed)
    fr = np.flatnonzero(free)
    if k % 4 == 0:
        return np.zeros(free.size, np.uint8)
    if k % 4 == 1:
        pen = rs.randint(0, 2, size=free.size).astype(np.uint8)
    elif k % 4 == 2:
        pen = rs.randint(0, 32, size=free.size).astype(np.uint8)
        pen[fr[rs.randint(len(fr))]] = 31
    else:
        return clearance_pen(free, dims)[1]
    pen[free == 0] = 255
    return pen


def same_paths(a, b):
    return len(a) == len(b) and all((p is None and q is None) or (p is not None and q is not None and np.array_equal(p, q)) for p, q in zip(a, b))


# ------------------------------------------------------------------ 1. word edges and small boxes, every step triple and penalty pattern
@functools.lru_cache(maxsize=None)
def box_case(k):
    """(dims, step, free, pen, sources, fields, starts, ends, (dist, node counts, paths)) of box k: test_gpu_chamfer's boxes and pairs with a penalty pattern"""
    dims, occ = BOXES[k]
    step = STEPS[k % len(STEPS)]
    seed = dims[0] * 1000 + dims[1] * 10 + dims[2]
    free, srcs = random_box(dims, occ, seed=seed)
    pen = pattern(k, free, dims, seed + 1)
    want = CW.fields(free, step, pen, dims, srcs)
    starts, ends = list(srcs), list(srcs[::-1])
    for i in range(min(3, len(srcs))):
        starts.append(srcs[i])
        ends.append(int(np.argmax(want[i])))
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    return dims, step, free, pen, srcs, want, starts, ends, CW.paths(free, step, pen, dims, starts, ends)


@pytest.mark.parametrize("k", range(len(BOXES)), ids=["x".join(map(str, b[0])) for b in BOXES])
def test_fields_matrix_and_paths_on_random_boxes(ctx, k):
    dims, step, free, pen, srcs, want, starts, ends, (w_dist, w_len, w_paths) = box_case(k)
    g = grid_of(ctx, free, dims)
    if k % 4 == 3:
        assert np.array_equal(g.clearance_costs([1, 4, 9]), clearance_pen(free, dims)[0]), "the pattern is the device's own clearance costs"
    got = g.chamfer_weighted_fields(step, pen, srcs)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(g.chamfer_weighted_matrix(step, pen, srcs), want[:, srcs])
    dist, lens, paths = api.chamfer_weighted_paths(g, step, pen, starts, ends)
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    assert same_paths(paths, w_paths)
    g.close()


def test_the_boxes_exercise_the_penalties():
    """over the boxes above, by the restatement alone (nothing here depends on the order the tests ran in)"""
    by_class = np.zeros(3, np.int64)
    differs = top_entered = 0
    for k in range(len(BOXES)):
        dims, step, free, pen, srcs, want, starts, ends, (_, _, new) = box_case(k)
        plain = C.paths(free, step, dims, starts, ends)[2]
        top = int(pen[free != 0].max())
        for p, q in zip(new, plain):
            if p is None:
                continue
            by_class += C.moves_by_class(dims, p)
            differs += not np.array_equal(p, q)
            top_entered += bool(top > 0 and (pen[p[1:]] == top).any())
        if k % 4 == 2:
            assert top == 31
    assert by_class[1] >= 1 and by_class[2] >= 1, "edge and corner moves occur"
    assert differs >= 1, "a path differs from the zero-penalty path of its pair"
    assert top_entered >= 1, "a voxel with the largest penalty is entered"


# ------------------------------------------------------------------ 2. the identities on the device
def test_identity_a_zero_penalties_are_the_bytes_of_the_chamfer_calls(ctx):
    for n, (dims, occ, seed) in enumerate((((130, 9, 7), 0.3, 1), ((64, 11, 5), 0.25, 2), ((67, 1, 1), 0.0, 3))):
        free, srcs = random_box(dims, occ, seed)
        pen = np.where(free != 0, 0, 255).astype(np.uint8)
        g = grid_of(ctx, free, dims)
        for step in (STEPS[2 * n], STEPS[2 * n + 1]):
            assert g.chamfer_weighted_fields(step, pen, srcs).tobytes() == g.chamfer_fields(step, srcs).tobytes()
            assert g.chamfer_weighted_matrix(step, pen, srcs).tobytes() == g.chamfer_matrix(step, srcs).tobytes()
            a = api.chamfer_weighted_paths(g, step, pen, srcs, srcs[::-1])
            b = api.chamfer_paths(g, step, srcs, srcs[::-1])
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[0] > 0).any()
            assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(a[2], b[2]))
        g.close()


def test_identity_b_a_constant_penalty_is_a_larger_step(ctx):
    dims = (129, 7, 5)
    free, srcs = random_box(dims, 0.25, 11)
    g = grid_of(ctx, free, dims)
    for step, c in (((3, 4, 5), 11), ((1, 1, 1), 15), ((5, 7, 9), 7), ((2, 3, 1), 13)):
        pen = np.where(free != 0, c, 255).astype(np.uint8)
        up = tuple(s + c for s in step)
        assert max(up) <= C.STEP_MAX
        assert g.chamfer_weighted_fields(step, pen, srcs).tobytes() == g.chamfer_fields(up, srcs).tobytes()
        assert g.chamfer_weighted_matrix(step, pen, srcs).tobytes() == g.chamfer_matrix(up, srcs).tobytes()
        a = api.chamfer_weighted_paths(g, step, pen, srcs, srcs[::-1])
        b = api.chamfer_paths(g, up, srcs, srcs[::-1])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(a[2], b[2]))
    g.close()


def test_identity_c_the_asymmetry_of_the_matrix(ctx):
    dims = (97, 6, 4)
    free, srcs = random_box(dims, 0.2, 21)
    rs = np.random.RandomState(5)
    pen = rs.randint(0, 32, size=free.size).astype(np.uint8)
    pen[srcs[0]] = 31                                     # a source whose own penalty is 31: not paid at the start
    pen[srcs[1]] = 0
    pen[free == 0] = 255
    cand = np.flatnonzero(free)
    pts = np.array(list(dict.fromkeys(srcs + [int(v) for v in cand[rs.randint(len(cand), size=8)]])), np.int64)
    g = grid_of(ctx, free, dims)
    for step in ((3, 4, 5), (16, 1, 7)):
        m = g.chamfer_weighted_matrix(step, pen, pts).astype(np.int64)
        f = g.chamfer_weighted_fields(step, pen, pts)
        assert np.array_equal(m, f[:, pts]), "fields and matrix are two routes to the same numbers"
        if step == (3, 4, 5):
            assert np.array_equal(m, CW.matrix(free, step, pen, dims, pts))
        assert (np.diag(m) == 0).all() and np.array_equal(m >= 0, (m >= 0).T), "reachability is symmetric"
        both = m >= 0
        pp = pen[pts].astype(np.int64)
        assert np.array_equal((m - m.T)[both], (pp[None, :] - pp[:, None])[both])
        assert (m != m.T).any() and both.sum() > len(pts) ** 2 // 2
        pocket = int(np.flatnonzero(pts == srcs[4])[0])
        assert (np.delete(m[pocket], pocket) == CW.NONE).all() and (np.delete(m[:, pocket], pocket) == CW.NONE).all()
    g.close()


# ------------------------------------------------------------------ 3. hand cases
def test_hand_cases(ctx):
    for name, free, step, pen, dims, src, want, want_paths in CW.hand_cases():
        g = grid_of(ctx, free, dims)
        f = g.chamfer_weighted_fields(step, pen, [src])[0]
        for v, k in want.items():
            assert f[v] == k, (name, v)
        assert np.array_equal(f, CW.field(free, step, pen, dims, src)), name
        ends = list(want_paths)
        d, n, p = api.chamfer_weighted_paths(g, step, pen, [src] * len(ends), ends)
        for e, q, dd, nn in zip(ends, p, d, n):
            assert q.tolist() == want_paths[e] and dd == want[e] and nn == len(want_paths[e]), (name, e)
        g.close()


def test_occupied_voxels_may_carry_any_byte(ctx):
    dims = (65, 5, 3)
    free, srcs = random_box(dims, 0.3, 41)
    pen = np.random.RandomState(2).randint(0, 32, size=free.size).astype(np.uint8)
    a, b = pen.copy(), pen.copy()
    a[free == 0], b[free == 0] = 255, 0
    g = grid_of(ctx, free, dims)
    want = CW.fields(free, (3, 4, 5), b, dims, srcs)
    assert np.array_equal(g.chamfer_weighted_fields((3, 4, 5), a, srcs), want)
    assert np.array_equal(g.chamfer_weighted_fields((3, 4, 5), b, srcs), want)
    g.close()


def test_serpentine_beyond_16_bits(ctx):
    """600 x 66 x 1, a wall on every second row with its gap at alternating ends: 19 833 free voxels in one line.  Every diagonal at a
    turn spans an occupied voxel, so with {4, 5, 6} the distance along the line is 4 * hops + the penalties entered: beyond 65 535."""
    nx, ny = 600, 66
    dims = (nx, ny, 1)
    step = (4, 5, 6)
    free = G.serpentine(nx, ny)
    hops = G.queue_field(free, dims, 0)
    n_free = int(free.sum())
    line = np.argsort(np.where(hops >= 0, hops, 1 << 30), kind="stable")[:n_free]
    pen = np.where(free != 0, np.random.RandomState(3).randint(0, 3, size=free.size), 255).astype(np.uint8)
    along = np.concatenate([[0], np.cumsum(4 + pen[line[1:]].astype(np.int64))])
    want = np.full(free.size, CW.NONE, np.int32)
    want[line] = along
    far, mid = int(line[-1]), int(line[7001])
    assert want[far] > 79328 > 65535
    g = grid_of(ctx, free, dims)
    f = g.chamfer_weighted_fields(step, pen, [0])[0]
    assert np.array_equal(f, want)
    d, n, p = api.chamfer_weighted_paths(g, step, pen, [0, far], [far, mid])
    back = int(want[far] - want[mid] - pen[far] + pen[mid])           # the line walked the other way: identity (c) on a part of it
    assert d.tolist() == [int(want[far]), back] and n.tolist() == [n_free, n_free - 7001]
    assert np.array_equal(p[0], line) and np.array_equal(p[1], line[7001:][::-1])
    g.close()


# ------------------------------------------------------------------ 4. the paths protocol
def _raw_paths(ctx, g, step, pen, starts, ends, off, ids, dist, lens):
    step = np.asarray(step, np.int32)
    return ctx.lib.wa_grid_chamfer_weighted_paths(g.h, P(step), P(pen), P(starts), P(ends), len(starts), P(off), P(ids), P(dist), P(lens))


def test_paths_protocol_and_clearance(ctx):
    dims = (67, 11, 9)
    step = (3, 4, 5)
    free, _ = random_box(dims, 0.2, seed=77)
    pen = clearance_pen(free, dims)[1]
    pocket = vid(dims, dims[0] // 2, dims[1] // 2, dims[2] // 2)
    rs = np.random.RandomState(4)
    moves = C._flat_moves(free, dims)
    reach = np.flatnonzero(CW.field(free, step, pen, dims, 0, moves) >= 0)
    s_pool = [0] + [int(v) for v in reach[rs.randint(len(reach), size=4)]]
    cand = np.flatnonzero(free)
    N = 30
    starts = [s_pool[k] for k in rs.randint(len(s_pool), size=N)]            # repeated starts, in no order
    ends = [int(v) for v in cand[rs.randint(len(cand), size=N)]]
    starts[7], ends[7] = s_pool[2], s_pool[2]                                # start == end
    starts[20], ends[20] = s_pool[1], pocket                                 # unreachable, in the middle of the batch
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    w_dist, w_len, w_paths = CW.paths(free, step, pen, dims, starts, ends)
    assert w_dist[20] == CW.NONE and w_len[20] == 0 and w_dist[7] == 0 and w_len[7] == 1 and (w_len > 15).sum() > 5
    g = grid_of(ctx, free, dims)
    dist, lens, paths = api.chamfer_weighted_paths(g, step, pen, starts, ends)
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len) and same_paths(paths, w_paths)
    for k in range(N):
        if w_dist[k] >= 0:
            C.check_path(free, dims, paths[k], int(starts[k]), int(ends[k]))
            assert CW.path_cost(step, pen, dims, paths[k]) == dist[k]
    # no returned path has a hit in wa_traj_clearance: unit-spaced grid, nodes map to themselves
    for k in np.argsort(-w_len)[:6]:
        p = paths[int(k)]
        xyz = np.stack([p % dims[0], (p // dims[0]) % dims[1], p // (dims[0] * dims[1])], axis=1).astype(np.float32)
        t = api.Trajectory.from_points(ctx, xyz)
        ids, _, hit, summary = t.clearance(g)
        assert np.array_equal(ids, p) and summary["n_hit"] == 0 and summary["n_outside"] == 0 and not hit.any()
        t.close()
    # the raw call: ranges with slack, a sentinel everywhere, nothing written behind a path or into the unreachable pair's range
    cap = w_len.astype(np.int64) + 3
    off = np.concatenate([[5], 5 + np.cumsum(cap)]).astype(np.int64)
    ids = np.full(int(off[-1]) + 4, SENT, np.int64)
    d2, l2 = np.full(N, SENT, np.int32), np.full(N, SENT, np.int32)
    assert _raw_paths(ctx, g, step, pen, starts, ends, off, ids, d2, l2) == 0
    assert np.array_equal(d2, w_dist) and np.array_equal(l2, w_len)
    assert (ids[:5] == SENT).all() and (ids[off[-1]:] == SENT).all()
    for k in range(N):
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
    d3, l3 = np.full(N, SENT, np.int32), np.full(N, SENT, np.int32)
    assert _raw_paths(ctx, g, step, pen, starts, ends, off2, ids2, d3, l3) == CAPACITY
    assert np.array_equal(d3, w_dist) and np.array_equal(l3, w_len), "dist_out and len_out are filled for every pair, also on WA_ERR_CAPACITY"
    assert (ids2[off2[k_short]:off2[k_short + 1]] == SENT).all(), "nothing is written for the pair that does not fit"
    for k in range(N):
        if k != k_short and w_dist[k] >= 0:
            assert np.array_equal(ids2[off2[k]:off2[k + 1]], w_paths[k])
    cap2[k_short] += 1                                                       # sized from len_out: the second call succeeds
    off3 = np.concatenate([[0], np.cumsum(cap2)]).astype(np.int64)
    ids3 = np.full(int(off3[-1]) + 1, SENT, np.int64)
    assert _raw_paths(ctx, g, step, pen, starts, ends, off3, ids3, d3, l3) == 0
    assert np.array_equal(ids3[off3[k_short]:off3[k_short + 1]], w_paths[k_short])
    g.close()


# ------------------------------------------------------------------ 5. chunking and repeatability
def chunk_scene():
    dims = (70, 9, 6)
    free, srcs = random_box(dims, 0.2, seed=5)
    pen = np.where(free != 0, np.random.RandomState(6).randint(0, 32, size=free.size), 255).astype(np.uint8)
    return dims, (2, 3, 16), free, pen, srcs


def digests(g, step, pen, srcs):
    H = lambda b: hashlib.blake2b(b, digest_size=16).hexdigest()
    d, n, p = api.chamfer_weighted_paths(g, step, pen, srcs, srcs[::-1])
    return [H(g.chamfer_weighted_fields(step, pen, srcs).tobytes()), H(g.chamfer_weighted_matrix(step, pen, srcs).tobytes()),
            H(d.tobytes() + n.tobytes() + b"".join(b"" if q is None else q.tobytes() for q in p))]


def test_results_do_not_depend_on_the_chunking(ctx):
    """the same sources one per chunk (WA_GEO_CHUNK=1 in a fresh child process) and all in one launch"""
    dims, step, free, pen, srcs = chunk_scene()
    g = grid_of(ctx, free, dims)
    here = digests(g, step, pen, srcs)
    assert (g.chamfer_weighted_matrix(step, pen, srcs) > 0).any()
    g.close()
    child = ("import sys; sys.path[:0] = [%r, %r]\n"
             "from welding_robot_amd import api\n"
             "from test_gpu_chamfer_weighted import chunk_scene, digests, grid_of\n"
             "dims, step, free, pen, srcs = chunk_scene()\n"
             "c = api.Context(0); g = grid_of(c, free, dims)\n"
             "print('digest', *digests(g, step, pen, srcs))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    assert line[1:] == here


def test_same_bytes_twice_and_two_contexts(ctx):
    dims, step, free, pen, srcs = chunk_scene()
    other = api.Context(0)
    g, g2 = grid_of(ctx, free, dims), grid_of(other, free, dims)
    a = digests(g, step, pen, srcs)
    b = digests(g2, step, pen, srcs)
    # other penalties and steps on the same grid in between: nothing of a call is kept
    assert g.chamfer_weighted_fields((1, 1, 1), np.zeros(free.size, np.uint8), srcs).tobytes() == g.chamfer_fields((1, 1, 1), srcs).tobytes()
    assert digests(g, step, pen, srcs) == a == b
    assert np.array_equal(g2.chamfer_weighted_fields(step, pen, srcs), CW.fields(free, step, pen, dims, srcs))
    g2.close()
    other.close()
    g.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments(ctx):
    dims = (9, 4, 3)
    free = np.ones(108, np.uint8)
    free[50] = 0
    g = grid_of(ctx, free, dims)
    lib = ctx.lib
    out = np.full(4 * 108, SENT, np.int32)
    lens = np.full(8, SENT, np.int32)
    ids_out = np.full(64, SENT, np.int64)
    off = np.array([0, 30, 60], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ok_ids = i64(0, 107)
    ok_step = np.array([3, 4, 5], np.int32)
    ok_pen = np.full(108, 2, np.uint8)
    ok_pen[50] = 255

    def untouched():
        return (out == SENT).all() and (ids_out == SENT).all() and (lens == SENT).all()

    def both_paths(step, pen, a, b, cnt, off_=off):
        return (lib.wa_grid_chamfer_weighted_paths(g.h, step, pen, a, b, cnt, P(off_), P(ids_out), P(out), P(lens)),
                lib.wa_grid_chamfer_weighted_paths(g.h, step, pen, b, a, cnt, P(off_), P(ids_out), P(out), P(lens)))

    def all_three(step, pen, a, b, cnt):
        return (lib.wa_grid_chamfer_weighted_fields(g.h, step, pen, a, cnt, P(out)),
                lib.wa_grid_chamfer_weighted_matrix(g.h, step, pen, a, cnt, P(out))) + both_paths(step, pen, a, b, cnt)

    # everything the chamfer calls refuse: ids occupied, outside (above, below, far above)
    for bad in (i64(0, 50), i64(0, 108), i64(-1, 0), i64(0, 1 << 40)):
        assert all_three(P(ok_step), P(ok_pen), P(bad), P(ok_ids), 2) == (ARG,) * 4 and untouched()
    # steps: 0, above WA_STEP_MAX, negative, in every position
    for k in range(3):
        for v in (0, 17, -1):
            bad_step = ok_step.copy()
            bad_step[k] = v
            assert all_three(P(bad_step), P(ok_pen), P(ok_ids), P(ok_ids), 2) == (ARG,) * 4 and untouched()
            assert b"step" in lib.wa_last_error(ctx.h)
    # a free voxel above WA_PEN_MAX (32, 255), wherever it lies
    for v, where in ((32, 0), (255, 107), (32, 49)):
        bad_pen = ok_pen.copy()
        bad_pen[where] = v
        assert all_three(P(ok_step), P(bad_pen), P(ok_ids), P(ok_ids), 2) == (ARG,) * 4 and untouched()
        assert b"WA_PEN_MAX" in lib.wa_last_error(ctx.h)
    # negative counts, NULL arrays (pen included, also with a count of 0), NULL outputs, decreasing offsets
    assert all_three(P(ok_step), P(ok_pen), P(ok_ids), P(ok_ids), -1) == (ARG,) * 4
    for cnt in (0, 2):
        assert all_three(None, P(ok_pen), P(ok_ids), P(ok_ids), cnt) == (ARG,) * 4
        assert all_three(P(ok_step), None, P(ok_ids), P(ok_ids), cnt) == (ARG,) * 4
        assert all_three(P(ok_step), P(ok_pen), None, None, cnt) == (ARG,) * 4
        assert both_paths(P(ok_step), P(ok_pen), P(ok_ids), None, cnt) == (ARG,) * 2
        assert lib.wa_grid_chamfer_weighted_fields(g.h, P(ok_step), P(ok_pen), P(ok_ids), cnt, None) == ARG
        assert lib.wa_grid_chamfer_weighted_matrix(g.h, P(ok_step), P(ok_pen), P(ok_ids), cnt, None) == ARG
        for k in range(4):
            a = [P(off), P(ids_out), P(out), P(lens)]
            a[k] = None
            assert lib.wa_grid_chamfer_weighted_paths(g.h, P(ok_step), P(ok_pen), P(ok_ids), P(ok_ids), cnt, *a) == ARG
    down = np.array([0, 30, 29], np.int64)
    assert both_paths(P(ok_step), P(ok_pen), P(ok_ids), P(ok_ids), 2, down) == (ARG,) * 2
    assert untouched()
    # counts of zero with valid pointers succeed, write nothing and do not look at pen (here: one that would be refused)
    bad_pen = np.full(108, 255, np.uint8)
    assert all_three(P(ok_step), P(bad_pen), P(ok_ids), P(ok_ids), 0) == (0,) * 4 and untouched()
    # and everything still works: (8, 3, 2) apart: 3 * 5 + 4 * 1 + 5 * 2 = 29 in 5 + 1 + 2 moves, 2 per voxel entered
    assert np.array_equal(g.occupancy(), free)
    assert g.chamfer_weighted_matrix(ok_step, ok_pen, ok_ids).tolist() == [[0, 29 + 16], [29 + 16, 0]]
    g.close()


def test_a_grid_whose_distances_might_not_fit_int32_is_refused(ctx):
    """1024 x 1024 x 44, all free: the fewest slabs for which (16 + 31) * (n - 1) > 2^31 - 1.  Step {16, 16, 16} alone fits (the chamfer
    calls accept it), penalty 30 fits, penalty 31 on one free voxel does not.  The refusal needs the largest penalty present, so it comes
    once the penalties are uploaded and packed, and before any search: the call that is accepted below does everything a refused call
    does and then runs the smallest search there is on this grid (one point, whose row is full at level 1: the buffers of one source,
    their clearing and one block of launches), so a refused call takes no longer than it does; the fastest of the three is compared,
    they do the same work (a search between the two points would run more than 16 000 levels)."""
    dims = (1024, 1024, 44)
    n = int(np.prod(dims))
    assert 47 * (n - 1) > 2 ** 31 - 1 >= 46 * (n - 1) and 47 * (n - 1024 * 1024 - 1) <= 2 ** 31 - 1
    free = np.ones(n, np.uint8)
    g = grid_of(ctx, free, dims)
    del free
    step = np.array([16, 16, 16], np.int32)
    pen = np.full(n, 30, np.uint8)
    pen[n // 2] = 31
    out, lens, ids_out = np.full(16, SENT, np.int32), np.full(4, SENT, np.int32), np.full(16, SENT, np.int64)
    pts = np.array([0, n - 1], np.int64)
    back = pts[::-1].copy()
    off = np.array([0, 8, 16], np.int64)
    lib = ctx.lib
    assert lib.wa_grid_chamfer_weighted_matrix(g.h, P(step), P(pen), P(pts[:1]), 1, P(out)) == ARG     # (the first call packs the occupancy)
    t_refused = []
    for call in (lambda: lib.wa_grid_chamfer_weighted_matrix(g.h, P(step), P(pen), P(pts), 2, P(out)),
                 lambda: lib.wa_grid_chamfer_weighted_fields(g.h, P(step), P(pen), P(pts), 2, P(out)),
                 lambda: lib.wa_grid_chamfer_weighted_paths(g.h, P(step), P(pen), P(pts), P(back), 2, P(off), P(ids_out), P(out), P(lens))):
        t0 = time.perf_counter()
        assert call() == ARG
        t_refused.append(time.perf_counter() - t0)
        assert b"int32" in lib.wa_last_error(ctx.h)
    assert (out == SENT).all() and (lens == SENT).all() and (ids_out == SENT).all()
    # one penalty less fits: a point's row is full at once
    pen[n // 2] = 30
    t0 = time.perf_counter()
    assert lib.wa_grid_chamfer_weighted_matrix(g.h, P(step), P(pen), P(pts[:1]), 1, P(out)) == 0 and out[0] == 0
    t_accepted = time.perf_counter() - t0
    print("\n  refused calls %s s, the accepted one-point call %.4f s" % (["%.4f" % t for t in t_refused], t_accepted))
    assert min(t_refused) <= t_accepted, "a refused call does less than the smallest accepted one"
    g.close()


# ------------------------------------------------------------------ 7. against the planners it combines
def test_no_dearer_than_the_chamfer_and_the_weighted_paths(ctx, capsys):
    """synth_grid(48), 8 points, bands 1, 4, 9, steps 3-4-5, gain 3.  A chamfer path and a 6-neighbour weighted path are both paths of
    the new graph, so under the new metric neither can be cheaper than the new distance of its pair."""
    n, step = 48, (3, 4, 5)
    dims = (n, n, n)
    free, cx, cy, cz, prec, wall = synth.synth_grid(n)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, 8, seed=7)
    cost = g.clearance_costs([1, 4, 9])
    pen = np.where(free != 0, 3 * (cost.astype(np.int64) - 1), 0).astype(np.uint8)
    ii, jj = np.triu_indices(8, 1)
    starts, ends = pts[ii], pts[jj]
    m = g.chamfer_weighted_matrix(step, pen, pts)
    dist, lens, new = api.chamfer_weighted_paths(g, step, pen, starts, ends)
    chm = api.chamfer_paths(g, step, starts, ends)[2]
    wgt = api.weighted_paths(g, cost, starts, ends)[2]
    d2 = g.distance_field()
    g.close()
    assert (dist >= 0).all() and np.array_equal(m[ii, jj], dist)
    for k in range(len(ii)):
        C.check_path(free, dims, new[k], int(starts[k]), int(ends[k]))
        assert CW.path_cost(step, pen, dims, new[k]) == dist[k]
        assert dist[k] <= CW.path_cost(step, pen, dims, chm[k]), k
        assert dist[k] <= CW.path_cost(step, pen, dims, wgt[k]), k
    near = lambda ps: int(sum((d2[p] <= 1).sum() for p in ps))
    moves = lambda ps: int(sum(C.path_cost(step, dims, p) for p in ps))
    with capsys.disabled():
        print("\n  48^3, 28 pairs: (nodes next to metal, step cost) new %s, chamfer %s, weighted %s"
              % ((near(new), moves(new)), (near(chm), moves(chm)), (near(wgt), moves(wgt))))


# ------------------------------------------------------------------ 8. the example
def run_plan_batch(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plan_batch_safe_diagonal_paths():
    out = run_plan_batch("--safe-paths", "3", "--diagonal-paths", "--shortcut")
    q = out["safe_diagonal_paths"]
    for key in ("step", "gain", "bands", "t_costs_s", "t_matrix_s", "t_paths_s", "nodes_total", "moves_by_class", "penalty_total",
                "nodes_next_to_metal", "n_hit", "n_hit_cubic", "shortened_length_total", "waypoints_total", "diagonal", "safe"):
        assert key in q, key
    assert q["step"] == [3, 4, 5] and q["gain"] == 3 and q["bands"] == [1, 4, 9]
    assert out["all_reached"] and q["n_hit"] == 0
    assert q["moves_by_class"][1] > 0 and sum(q["moves_by_class"]) == q["nodes_total"] - 28
    for other in ("diagonal", "safe"):
        for key in ("nodes_total", "moves_by_class", "penalty_total", "nodes_next_to_metal", "n_hit", "shortened_length_total"):
            assert key in q[other], (other, key)
    assert q["safe"]["moves_by_class"][1:] == [0, 0]
    assert "safe_paths" not in out and "diagonal_paths" not in out
    assert out["lattice_length_total"] >= out["shortened_length_total"] > 0


@pytest.mark.parametrize("flags, key", [(("--safe-paths", "3"), "safe_paths"), (("--diagonal-paths",), "diagonal_paths")])
def test_plan_batch_each_flag_alone_is_as_before(flags, key):
    out = run_plan_batch(*flags)
    assert key in out and "safe_diagonal_paths" not in out and out["all_reached"]


def test_plan_batch_refuses_a_gain_beyond_the_penalty_range():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "48", "--points", "8", "--safe-paths", "3",
                        "--diagonal-paths", "--safe-gain", "11"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 2 and "31" in r.stderr
