"""Red zones round every plain device block.  WA_DEV_GUARD=1 (csrc/weldacs.hip: dev_malloc / dev_free) allocates 4096 bytes in front of
and behind every block and fills them with WA_DEV_GUARD_BYTE; when the block is given back the device is waited for and both zones are
compared byte by byte.  A kernel that writes one element or one row past a hand-sized scratch buffer lands in the slack of the driver's
granule and changes nothing anybody reads: no other test sees it.  wa_ctx_guard_stats counts it, and counts the blocks that are live.

1. The mechanism: wa_ctx_guard_selftest writes ONE byte at a chosen offset of a guarded block of the library's own -- no kernel is
   altered to prove the check.  Every zone edge, at sizes round the < 16 -> 16 rounding and the zone's own 4096.
2. Tight sizes: every planner once where its buffers hold one element or end on an odd byte, on contexts that are poisoned as well,
   bit for bit against the restatement its own GPU test file uses (cases and scenes are imported from tests/test_gpu_poisoned_scratch.py
   and the families' files; none is restated here).  Every case: no damaged zone, blocks were checked, and behind close + trim the
   context holds as many blocks as before.

A fresh guarded context owns 0 blocks (measured on an MI355X): streams and events are no device blocks, and nothing is allocated
before the first call that needs it."""
import contextlib

import numpy as np
import pytest

import chamfer_ref as CH
import chamfer_weighted_ref as CW
import clearance_ref as CL
import geodesic_ref as G
import oracle_lib as O
import test_gpu_poisoned_scratch as P
import weighted_ref as W
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
Z = 4096
ARG, STATE = 1, 8
NOTHING = dict(dict.fromkeys(api.Context.GUARD_KEYS, 0), first_bytes=-1)


def damaged(s):
    return s["front_damaged"] + s["back_damaged"]


# ------------------------------------------------------------------ 1. the mechanism
def test_a_fresh_guarded_context_owns_no_block():
    c = P.make_ctx(WA_DEV_GUARD=1)
    try:
        assert c.guard_stats() == NOTHING
        c.trim()
        assert c.guard_stats() == NOTHING
    finally:
        c.close()


SIZES = [1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 1]


@pytest.mark.parametrize("n", SIZES)
def test_one_stray_byte_is_counted_once_and_where_it_fell(n):
    """a context per size, so that the block of this size is the FIRST damaged one and [6] / [7] are its own"""
    for off, front, back in ((-Z, 1, 0), (-1, 1, 0), (n, 0, 1), (n + Z - 1, 0, 1)):
        c = P.make_ctx(WA_DEV_GUARD=1)
        try:
            c.guard_selftest(n, 0)
            c.guard_selftest(n, n - 1)          # inside the block: nothing to count
            s = c.guard_stats()
            assert s == dict(NOTHING, handed_out=2, checked=2), (n, s)
            c.guard_selftest(n, off)
            s = c.guard_stats()
            want = dict(NOTHING, handed_out=3, checked=3, front_damaged=front, back_damaged=back, first_bytes=n,
                        first_distance=off if off < 0 else off - n)
            assert s == want, (n, off, s)
        finally:
            c.close()


def test_counters_are_monotone_and_the_first_finding_stays():
    c = P.make_ctx(WA_DEV_GUARD=1, WA_DEV_GUARD_BYTE=0x3c, WA_DEV_POISON=1)
    try:
        free = P.occupancy((3, 5, 7))
        g = P.unit_grid(c, free, (3, 5, 7))          # live blocks of somebody else while the self-tests run
        live = c.guard_stats()
        assert live["live_blocks"] == 4 and live["live_bytes"] == 4 * (3 + 5 + 7) + 105, live
        prev = live
        for n, off in [(17, 17), (4097, -3), (1, 0), (16, Z + 15), (15, -Z)]:
            c.guard_selftest(n, off)
            s = c.guard_stats()
            for k in ("handed_out", "checked", "front_damaged", "back_damaged"):
                assert s[k] >= prev[k], (k, prev, s)
            assert s["handed_out"] == prev["handed_out"] + 1 and s["checked"] == prev["checked"] + 1
            assert (s["live_blocks"], s["live_bytes"]) == (live["live_blocks"], live["live_bytes"]), s
            assert (s["first_bytes"], s["first_distance"]) == (17, 0), s       # the first damaged block, not the last
            prev = s
        assert (prev["front_damaged"], prev["back_damaged"]) == (2, 2)
        assert np.array_equal(g.occupancy(), free)
        g.close()
        s = c.guard_stats()
        assert s["live_blocks"] == 0 and s["live_bytes"] == 0 and damaged(s) == 4, s
        assert c.poison_stats()["plain_bytes"] >= 17 + 4097 + 1 + 16 + 15       # (the poison covers the block, never its zones)
    finally:
        c.close()


def test_selftest_refuses_what_leaves_the_zones_and_plain_contexts():
    c = P.make_ctx(WA_DEV_GUARD=1)
    try:
        for n, off in [(16, -Z - 1), (16, 16 + Z), (1, 1 + Z), (-1, 0)]:
            assert c.lib.wa_ctx_guard_selftest(c.h, n, off) == ARG, (n, off)
        assert c.lib.wa_ctx_guard_stats(c.h, None) == ARG
        assert c.guard_stats() == NOTHING
    finally:
        c.close()
    c = P.make_ctx(WA_DEV_GUARD=0)
    try:
        for n, off in [(16, 0), (16, 16), (16, -Z - 1)]:
            assert c.lib.wa_ctx_guard_selftest(c.h, n, off) == STATE, (n, off)
        assert c.guard_stats() == NOTHING
    finally:
        c.close()


# ------------------------------------------------------------------ 2. tight sizes
@pytest.fixture(scope="module", params=P.BYTES, ids=lambda b: "byte%02x" % b)
def ctx(request):
    """guarded and poisoned, like the two contexts of tests/test_gpu_poisoned_scratch.py (0xff with zones of 0xa5, 0x55 with 0x3c)"""
    env = {"WA_DEV_POISON": 1, "WA_DEV_POISON_BYTE": request.param, "WA_DEV_GUARD": 1, "WA_DEV_GUARD_BYTE": P.GUARD_BYTE[request.param]}
    c = P.make_ctx(**env)
    yield c
    c.trim()
    s = c.guard_stats()
    c.close()
    assert s["live_blocks"] == 0 and damaged(s) == 0, s


@contextlib.contextmanager
def tight(ctx, blocks=True):
    """no zone damaged, blocks freed and checked (blocks=False: the call is known to take none, and takes none), and behind close + trim
    as many live blocks as before"""
    ctx.trim()
    before = ctx.guard_stats()
    assert damaged(before) == 0, before
    yield
    ctx.trim()
    after = ctx.guard_stats()
    assert damaged(after) == 0, after
    assert (after["checked"] > before["checked"]) if blocks else (after["handed_out"] == before["handed_out"]), (before, after)
    assert (after["live_blocks"], after["live_bytes"]) == (before["live_blocks"], before["live_bytes"]), (before, after)


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7)], ids=P.dims_id)
def test_grids_of_one_and_of_105_voxels(ctx, dims):
    free = P.occupancy(dims)
    d2 = CL.edt_separable(free, *dims)
    keep = np.array([0], np.int64)
    want = CL.inflate(free, d2, *dims, 1.0, keep)
    with tight(ctx):
        g = P.unit_grid(ctx, free, dims)
        assert np.array_equal(g.occupancy(), free) and g.n_free == int(free.sum())
        assert np.array_equal(g.distance_field(), d2)
        gi = g.inflate(1.0, keep)
        assert np.array_equal(gi.occupancy(), want) and gi.n_free == int(want.sum())
        gi.close()
        g.close()


@pytest.mark.parametrize("n_pts", [17, 33])
def test_resolve_on_the_device(ctx, n_pts):
    dims = (3, 5, 7)
    pts, want = P.resolve_case(dims, n_pts)
    with tight(ctx):
        g = P.unit_grid(ctx, P.occupancy(dims), dims)
        assert np.array_equal(g.resolve(pts), want)
        g.close()


SEARCH_DIMS = (65, 5, 3)      # 975 voxels: int32 fields of 3 900 bytes, bitmap rows of two words; the smallest box of the searches' cases


def few_pairs(srcs):
    return srcs + srcs[:1], srcs[::-1] + srcs[:1]


@pytest.mark.parametrize("ns", [1, 3])
def test_searches_with_one_and_three_sources_in_chunks_of_two(ctx, ns):
    dims = SEARCH_DIMS
    free, all_srcs = P.search_box(dims)
    srcs = all_srcs[:ns]
    s, e = few_pairs(srcs)
    cost = P.weighted_want(dims)[0]
    step, pen = P.chamfer_weighted_want(dims)[:2]
    with tight(ctx), P.environ(WA_GEO_CHUNK=2):
        g = P.unit_grid(ctx, free, dims)
        want = G.fields(free, dims, srcs)
        assert np.array_equal(g.geodesic_fields(srcs), want) and np.array_equal(g.geodesic_matrix(srcs), want[:, srcs])
        hops, paths = api.geodesic_paths(g, s, e)
        w_hops, w_paths = G.paths(free, dims, s, e)
        assert np.array_equal(hops, w_hops)
        P.same_paths(paths, w_paths)

        want = W.fields(free, cost, dims, srcs)
        assert np.array_equal(g.weighted_fields(cost, srcs), want) and np.array_equal(g.weighted_matrix(cost, srcs), want[:, srcs])
        dist, lens, paths = api.weighted_paths(g, cost, s, e)
        w_dist, w_len, w_paths = W.paths(free, cost, dims, s, e)
        assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
        P.same_paths(paths, w_paths)

        want = CH.fields(free, step, dims, srcs)
        assert np.array_equal(g.chamfer_fields(step, srcs), want) and np.array_equal(g.chamfer_matrix(step, srcs), want[:, srcs])
        dist, lens, paths = api.chamfer_paths(g, step, s, e)
        w_dist, w_len, w_paths = CH.paths(free, step, dims, s, e)
        assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
        P.same_paths(paths, w_paths)

        want = CW.fields(free, step, pen, dims, srcs)
        assert np.array_equal(g.chamfer_weighted_fields(step, pen, srcs), want)
        assert np.array_equal(g.chamfer_weighted_matrix(step, pen, srcs), want[:, srcs])
        dist, lens, paths = api.chamfer_weighted_paths(g, step, pen, s, e)
        w_dist, w_len, w_paths = CW.paths(free, step, pen, dims, s, e)
        assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
        P.same_paths(paths, w_paths)
        g.close()


@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("family", ["pose_hops", "pose_weighted", "pose_diag"])
def test_pose_searches_with_one_direction_and_a_second_mask_word(ctx, family, K):
    with tight(ctx):
        getattr(P, "test_" + family)(ctx, K)


# (K, nx, beads): one direction, a second mask word, one bead.  The case's thresholds are 1, K // 2, K: K = 1 has a threshold of 0.
@pytest.mark.parametrize("K,nx,n_beads", [(1, 63, 4), (65, 63, 1), (65, 65, 4)])
def test_reach_fit_penalties(ctx, K, nx, n_beads):
    with tight(ctx):
        P.test_reach_fit_penalties(ctx, K, nx, n_beads)


@pytest.mark.parametrize("span", [128, 7])
def test_shortcut_batch_of_257_paths_of_one_and_two_nodes(ctx, span):
    import shortcut_ref as S
    free, (nx, ny, nz), axes, _, _ = P.shortcut_case()
    at = lambda i: nx * ny + i % 64 + nx * (i // 64 % ny)   # noqa: E731  (the open slab z = 1; x < 64, so that at(i) + 1 is its neighbour)
    paths = [np.array([at(i)] if i % 2 else [at(i), at(i) + 1], np.int64) for i in range(257)]
    cache = {}
    want = [S.shortcut(free, nx, ny, *axes, p, span, cache) for p in paths]
    with tight(ctx):
        g = api.Grid.from_occupancy(ctx, free, *axes, 1.0, 0)
        wps, lengths = api.shortcut_paths(g, paths, span)
        for p, w, ln, (ww, wl) in zip(paths, wps, lengths, want):
            assert np.array_equal(w, p[ww]) and np.float64(ln).view(np.uint64) == np.float64(wl).view(np.uint64)
        wps, lengths = api.shortcut_paths(g, paths[1:2], span)      # a batch of one path of one node
        assert np.array_equal(wps[0], paths[1]) and lengths[0] == 0.0
        g.close()


def test_pose_shortcut_batch_of_257_paths_of_one_and_two_nodes(ctx):
    from test_gpu_pose_shortcut import check
    c, sc, paths, kss, _ = P.pose_shortcut_case()
    assert len(paths[3]) == 1 and len(paths[4]) == 2
    many = ([paths[3], paths[4]] * 129)[:257]
    many_ks = ([kss[3], kss[4]] * 129)[:257]
    with tight(ctx):
        g = P.pose_grid(ctx, c)
        check(g, sc, many, many_ks, 24, "257 short paths")
        check(g, sc, many[:1], many_ks[:1], 24, "one path of one node")
        g.close()


def test_stitch_one_node_and_ragged_segments(ctx):
    from test_gpu_trajectory import bits
    dims = (3, 5, 7)
    free = P.occupancy(dims)
    ax = [np.arange(d, dtype=np.float32) for d in dims]
    ids = np.flatnonzero(free).astype(np.int64)
    with tight(ctx):
        g = P.unit_grid(ctx, free, dims)
        for segs, rev in (([ids[:1]], None), ([ids[:3], ids[:0], ids[5:6], ids[7:14]], np.array([1, 0, 1, 0], np.uint8))):
            t = api.Trajectory.stitch(g, segs, rev)
            off = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
            want = O.stitch_segments(np.concatenate(segs), off, rev if rev is not None else np.zeros(len(segs), np.uint8), dims[0], dims[1], *ax)
            assert np.array_equal(bits(t.points()), bits(want))
            t.close()
        g.close()


# (dim, degree, ci, cf, n_middle, count): degree 0 and 7, dim 1 and 16, 1 and 257 parameters / samples
@pytest.mark.parametrize("dim,deg,ci,cf,n,count", [(1, 0, 0, 0, 1, 1), (16, 7, 7, 7, 1, 257), (1, 7, 3, 0, 5, 257), (16, 0, 0, 0, 257, 1)])
def test_bspline_eval_and_sample(ctx, dim, deg, ci, cf, n, count):
    from test_gpu_trajectory import bits
    rs = np.random.RandomState(dim * 100 + deg + count)
    mid = rs.uniform(-1, 1, size=(n, dim)).astype(np.float32)
    init, fin = rs.uniform(-1, 1, size=(ci + 1, dim)).astype(np.float32), rs.uniform(-1, 1, size=(cf + 1, dim)).astype(np.float32)
    tf = 7.5
    ob = O.Bspline(dim, deg, ci, cf, n)
    ob.set_param(init, fin, mid, tf)
    us = rs.uniform(-0.5, tf + 0.5, size=count).astype(np.float32)
    with tight(ctx):
        b = api.Bspline(ctx, dim, deg, ci, cf, n)
        b.set_param(init, fin, mid, tf)
        knots, cps = b.arrays()
        assert np.array_equal(bits(knots), bits(ob.knots)) and np.array_equal(bits(cps), bits(ob.cps))
        for der in sorted({0, min(1, deg), deg}):
            got, ok = b.eval(us, der)
            want, wok = ob.eval(us, der, prefill=0.0)
            assert np.array_equal(ok, wok) and np.array_equal(bits(got), bits(want)), der
            got, ok = b.sample(np.float32(-0.1), np.float32(1.02 * tf / count), count, der)
            want, wok = ob.sample(np.float32(-0.1), np.float32(1.02 * tf / count), count, der, prefill=0.0)
            assert np.array_equal(ok, wok) and np.array_equal(bits(got), bits(want)), der
        b.close()


def test_clearance_of_1_2_and_257_samples(ctx):
    with tight(ctx):
        P.test_clearance_on_poisoned_memory(ctx, (65, 2, 3))


@pytest.mark.parametrize("n_legs", [1, 257])
def test_fit_and_pose_fit(ctx, n_legs):
    with tight(ctx):
        P.test_fit_refines_on_poisoned_memory(ctx, n_legs)
    with tight(ctx):
        P.test_pose_fit_leg_counts_around_the_block(ctx, n_legs)


@pytest.mark.parametrize("n", [2, 2049])
def test_retime_ticks_and_stops(ctx, n):
    with tight(ctx):
        P.test_retime_stops_and_tick_axes(ctx, n)


@pytest.mark.parametrize("K,n_beads", [(1, 33), (65, 64)])
def test_torch_axes(ctx, K, n_beads):
    with tight(ctx):
        P.test_torch_axes_and_check(ctx, K, n_beads)


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_seam_tours_and_rules_of_one_and_two_seams(ctx, case):
    """(their scratch comes from the context's allocator: whole blocks of dev_malloc below 1 MiB, given back at once)"""
    assert P.SEAM_CASES[case][0] in (1, 2)
    with tight(ctx):
        P.test_seam_tours_and_rules(ctx, case)


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_seam_exact_programmes_of_one_two_and_three_seams(ctx, m, closed):
    import seamrules_ref as SR
    import seamtour_ref as ST
    from test_gpu_seamrules import kw_rules, rules_of
    from test_gpu_seamtour import euclid
    d = euclid(m, 900 + m)
    b, a, fx = rules_of("r", m, 17 + m, closed)
    want, want_rules = ST.seam_tour_exact(d, m, closed), SR.seam_tour_rules_exact(d, m, closed=closed, **kw_rules(b, a, fx))
    # one closed seam: the programmes have no cell beside the anchor and take no device block; the smallest job that does is M = 2
    with tight(ctx, blocks=not (m == 1 and closed)):
        got = api.seam_tour_exact(ctx, d, closed)
        assert got["cost_q"] == want["cost_q"] and np.array_equal(got["order"], want["order"]) and np.array_equal(got["dir"], want["dir"])
        got = api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)
        assert got["cost_q"] == want_rules["cost_q"]
        assert np.array_equal(got["order"], want_rules["order"]) and np.array_equal(got["dir"], want_rules["dir"])


@pytest.mark.parametrize("variant", [v for v, n in P.GTSP_SMALLEST.items() if n == 2])
def test_gtsp_of_two_and_three_cities(ctx, variant):
    """every kernel the dispatch can select at these sizes: the wavefront kernel, the one-wavefront fast kernel, the generic one"""
    with tight(ctx):
        P.run_gtsp(ctx, variant, P.gtsp_case(variant, (2, 3)))
