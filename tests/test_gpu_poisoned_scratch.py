"""The planning calls on hostile memory.  WA_DEV_POISON=1 fills every device block the library allocates -- the plain ones of DevBuf /
dalloc / dev_malloc included -- with WA_DEV_POISON_BYTE before it is used (csrc/weldacs.hip, DESIGN "what each buffer starts with").
Fresh device memory reads 0, so a kernel that reads a word nobody wrote passes every other test of the suite; here it reads 0xff (-1,
WA_HOPS_NONE, all bits set) on one context and 0x55 (half-set bitmaps, large positive int32, finite floats) on the other.

Every test runs on both contexts, compares every returned array and summary BIT FOR BIT with the family's numpy restatement
(tests/*_ref.py) -- no tolerance anywhere in this file -- and asserts that wa_ctx_poison_stats' plain-allocator byte counter grew
during the call, so that no test is vacuous.  Shapes are the smallest that still have the edges where an unwritten word can be read:
rows of 65 and 130 voxels (a second / third bitmap word with 63 / 62 pad bits), last chunks that hold fewer sources than the chunk
before, node and leg counts around a block of 256.

The seam tours take all their scratch from the context's allocator (CtxBuf): their tests assert that allocator's counter instead.

Both contexts also run with WA_DEV_GUARD=1 (red zones of 4096 bytes round every dev_malloc block, compared when the block is freed:
csrc/weldacs.hip dev_free, tests/test_gpu_red_zones.py), with guard bytes 0xa5 and 0x3c: neither is a poison byte or 0, so a stray
write of any one constant damages a zone on at least one context, and a read that runs into a zone gets different bytes on the two.
Around every wrapped call blocks were freed and checked and no zone was damaged; every test gives back every block it took (the live
count behind close + trim is what it was before the test), the refused calls above all; at the end of the module a context holds what
a fresh one holds -- 0 blocks, measured on an MI355X (test_gpu_red_zones.test_a_fresh_guarded_context_owns_no_block) -- and no damaged
zone was ever counted.
DESIGN 3a reads every buffer of the families below at the desk: a poisoned index would be an access out of range, not a wrong answer."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chamfer_ref as CH
import chamfer_weighted_ref as CW
import clearance_ref as CL
import geodesic_ref as G
import weighted_ref as W
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ARG, CAPACITY = 1, 7
BYTES = (255, 85)
GUARD_BYTE = {255: 0xa5, 85: 0x3c}
FRESH_LIVE = 0      # blocks a freshly created guarded context owns


def make_ctx(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=BYTES, ids=lambda b: "byte%02x" % b)
def ctx(request):
    """the two poisoned contexts of this file, one after the other: 0xff (the knob's default) and 0x55, both with red zones.  Behind
    the module and a trim a context holds what a fresh guarded one holds: 0 live blocks, measured on an MI355X (a context owns a
    stream and no device block), and never counted a damaged zone."""
    env = {"WA_DEV_POISON": 1, "WA_DEV_GUARD": 1, "WA_DEV_GUARD_BYTE": GUARD_BYTE[request.param]}
    if request.param != 255:
        env["WA_DEV_POISON_BYTE"] = request.param
    c = make_ctx(**env)
    yield c
    c.trim()
    s = c.guard_stats()
    c.close()
    assert s["live_blocks"] == FRESH_LIVE and s["front_damaged"] + s["back_damaged"] == 0 and s["checked"] > 0, s


@pytest.fixture(autouse=True)
def every_block_comes_back(request):
    """the blocks of the context that are live behind trim: the same number before the test and after it has closed its handles"""
    if "ctx" not in request.fixturenames:
        yield
        return
    c = request.getfixturevalue("ctx")
    c.trim()
    before = c.guard_stats()
    yield
    c.trim()
    after = c.guard_stats()
    assert after["live_blocks"] == before["live_blocks"] and after["live_bytes"] == before["live_bytes"], (before, after)


@contextlib.contextmanager
def poisoned(ctx, which="plain"):
    """the calls inside allocated device blocks, and those were filled: plain ones (DevBuf / dalloc / dev_malloc) unless the family
    takes all of its scratch from the context's allocator (which="ctx": the seam tours' CtxBuf blocks)"""
    before, g_before = ctx.poison_stats(), ctx.guard_stats()
    yield
    after, g_after = ctx.poison_stats(), ctx.guard_stats()
    assert after[which + "_bytes"] > before[which + "_bytes"] and after[which + "_blocks"] > before[which + "_blocks"], (before, after)
    # ... and blocks were given back between their red zones, checked, with no byte of a zone changed
    assert g_after["checked"] > g_before["checked"] and g_after["front_damaged"] + g_after["back_damaged"] == 0, (g_before, g_after)


@contextlib.contextmanager
def environ(**env):
    """knobs the library reads per call (WA_GEO_CHUNK)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def unit_grid(ctx, free, dims):
    ax = lambda n: np.arange(n, dtype=np.float32)   # noqa: E731
    return api.Grid.from_occupancy(ctx, free, ax(dims[0]), ax(dims[1]), ax(dims[2]), 1.0, 0)


def vid(dims, x, y, z):
    return x + dims[0] * (y + dims[1] * z)


def same_paths(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, np.asarray(b, np.int64))


def test_counters_stay_zero_without_the_knob():
    c = make_ctx(WA_DEV_POISON=0)
    try:
        dims = (65, 5, 3)
        free, srcs = search_box(dims)
        g = unit_grid(c, free, dims)
        assert np.array_equal(g.geodesic_fields(srcs[:2]), G.fields(free, dims, srcs[:2]))
        g.distance_field()
        g.close()
        assert c.poison_stats() == {"ctx_blocks": 0, "ctx_bytes": 0, "plain_blocks": 0, "plain_bytes": 0}
        assert c.guard_stats() == dict(dict.fromkeys(api.Context.GUARD_KEYS, 0), first_bytes=-1)
        with pytest.raises(api.WeldacsError) as refused:
            c.guard_selftest(16, 16)
        assert refused.value.code == 8      # WA_ERR_STATE: no guarded block to damage on a plain context
        assert c.guard_stats() == dict(dict.fromkeys(api.Context.GUARD_KEYS, 0), first_bytes=-1)
    finally:
        c.close()


# ------------------------------------------------------------------ 1. grid build and the grid's cached state
@functools.lru_cache(None)
def occupancy(dims, occ=0.30):
    rs = np.random.RandomState(dims[0] * 100 + dims[1])
    free = (rs.uniform(size=int(np.prod(dims))) >= occ).astype(np.uint8)
    free[0] = free[-1] = 1
    free.setflags(write=False)
    return free


dims_id_early = lambda d: "x".join(map(str, d))   # noqa: E731


@functools.lru_cache(None)
def build_want(dims):
    free = occupancy(dims)
    return G.fields(free, dims, [0, int(np.prod(dims)) - 1]), CL.edt_separable(free, *dims)


@pytest.mark.parametrize("dims", [(65, 5, 3), (130, 4, 3)], ids=lambda d: "x".join(map(str, d)))
def test_grid_build_then_first_call(ctx, dims):
    """the FIRST call on a freshly built grid builds the grid's cached state on poisoned memory: a geodesic call packs the occupancy
    (fbits: the pad bits of every row must read occupied), a distance-field call builds d2 and the axis tables"""
    free = occupancy(dims)
    n = int(np.prod(dims))
    want_hops, want_d2 = build_want(dims)
    with poisoned(ctx):
        g = unit_grid(ctx, free, dims)
    assert np.array_equal(g.occupancy(), free) and g.n_free == int(free.sum())
    with poisoned(ctx):
        assert np.array_equal(g.geodesic_fields([0, n - 1]), want_hops)
    with poisoned(ctx):
        assert np.array_equal(g.distance_field(), want_d2)
    g.close()
    with poisoned(ctx):
        g = unit_grid(ctx, free, dims)
    with poisoned(ctx):
        assert np.array_equal(g.distance_field(), want_d2)
    with poisoned(ctx):
        assert np.array_equal(g.geodesic_matrix([0, n - 1]), want_hops[:, [0, n - 1]])
    g.close()


@functools.lru_cache(None)
def resolve_case(dims, n_pts=40):
    """40 points (more than the 16 the host mirror answers; tests/test_gpu_red_zones.py asks for 17 and 33): on nodes, between them, and far outside, where no voxel matches and the id stays
    -1 -- the value d_ids is memset to, which the 0x55 context tells from a fill that is missing.  The definition restated: the LAST
    free voxel in raster order within 1.2 * precision of the point on every axis (fp32 differences)."""
    free = occupancy(dims)
    rs = np.random.RandomState(5)
    pts = np.stack([rs.uniform(-1, d, n_pts) for d in dims], 1).astype(np.float32)
    pts[::4] = np.round(pts[::4])
    pts[1::8] += np.float32(500.0)
    t = np.float32(1.2 * 1.0)
    ax = [np.arange(d, dtype=np.float32) for d in dims]
    want = np.full(len(pts), -1, np.int64)
    for i, q in enumerate(pts):
        ok = [np.flatnonzero(np.abs(q[c] - ax[c]) < t) for c in range(3)]
        for z in ok[2]:
            for y in ok[1]:
                for x in ok[0]:
                    v = vid(dims, int(x), int(y), int(z))
                    if free[v] and v > want[i]:
                        want[i] = v
    assert n_pts != 40 or ((want < 0).sum() >= 5 and (want >= 0).sum() >= 20)
    assert (want < 0).any() and (want >= 0).any()
    return pts, want


@pytest.mark.parametrize("dims", [(65, 5, 3)], ids=dims_id_early)
def test_resolve_points_on_the_device(ctx, dims):
    pts, want = resolve_case(dims)
    g = unit_grid(ctx, occupancy(dims), dims)
    with poisoned(ctx):
        assert np.array_equal(g.resolve(pts), want)
    g.close()


def test_voxelise_cubic_on_poisoned_memory(ctx):
    import waf
    gold = waf.load(os.path.join(GOLD, "vox_cubic_p0219_w8.waf"))
    tris = api.stl_read_file(os.path.join(GOLD, "cubic.stl"))
    with poisoned(ctx):
        g = api.Grid.from_mesh(ctx, tris, float("0.0219"), int(gold["dims"][3]))
    assert (g.nx, g.ny, g.nz) == tuple(int(v) for v in gold["dims"][:3])
    occ = g.occupancy()
    assert np.array_equal(np.packbits(occ), gold["free_packed"]) and g.n_free == int(occ.sum())
    cx, cy, cz = g.coords()
    assert all(np.array_equal(a.view(np.uint32), np.asarray(gold[k], np.float32).view(np.uint32)) for a, k in ((cx, "cx"), (cy, "cy"), (cz, "cz")))
    g.close()


# ------------------------------------------------------------------ 2. the level driver: hops, weighted, chamfer, chamfer-weighted
@functools.lru_cache(None)
def search_box(dims, occ=0.30):
    """seeded occupancy with a one-voxel pocket at the centre (free, every face neighbour occupied: rings drain, *_NONE entries);
    7 sources -- the corners, the pocket, random free voxels -- so that WA_GEO_CHUNK=3 gives chunks of 3, 3 and 1"""
    nx, ny, nz = dims
    rs = np.random.RandomState(nx * 1000 + ny * 10 + nz)
    free = (rs.uniform(size=nx * ny * nz) >= occ).astype(np.uint8)
    corners = [vid(dims, 0, 0, 0), vid(dims, nx - 1, ny - 1, nz - 1), vid(dims, nx - 1, 0, 0), vid(dims, 0, ny - 1, nz - 1)]
    p = vid(dims, nx // 2, ny // 2, nz // 2)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y, z = nx // 2 + dx, ny // 2 + dy, nz // 2 + dz
                if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz:
                    free[vid(dims, x, y, z)] = 0      # (the whole shell: the pocket is closed to diagonal moves too)
    free[p] = 1
    free[corners] = 1
    cand = np.flatnonzero(free)
    srcs = list(dict.fromkeys(corners + [p] + [int(v) for v in cand[rs.randint(len(cand), size=12)]]))[:7]
    assert len(srcs) == 7
    free.setflags(write=False)
    return free, srcs


def pairs_of(free, srcs):
    """pairs for the _paths calls: every source as a start (two of them twice), ends among the sources, the pocket and far voxels"""
    cand = np.flatnonzero(free)
    starts = srcs + srcs[:2]
    ends = srcs[::-1] + [int(cand[len(cand) // 3]), int(cand[-2])]
    return starts, ends


SEARCH_DIMS = [(65, 5, 3), (130, 9, 7)]
dims_id = lambda d: "x".join(map(str, d))   # noqa: E731


@functools.lru_cache(None)
def hops_want(dims):
    free, srcs = search_box(dims)
    return G.fields(free, dims, srcs), G.paths(free, dims, *pairs_of(free, srcs))


@pytest.mark.parametrize("dims", SEARCH_DIMS, ids=dims_id)
def test_geodesic_in_three_chunks(ctx, dims):
    free, srcs = search_box(dims)
    want, (w_hops, w_paths) = hops_want(dims)
    assert (want[:, free != 0] == G.NONE).any()
    g = unit_grid(ctx, free, dims)
    with environ(WA_GEO_CHUNK=3), poisoned(ctx):
        assert np.array_equal(g.geodesic_fields(srcs), want)
        assert np.array_equal(g.geodesic_matrix(srcs), want[:, srcs])
        hops, paths = api.geodesic_paths(g, *pairs_of(free, srcs))
    assert np.array_equal(hops, w_hops)
    same_paths(paths, w_paths)
    g.close()


@functools.lru_cache(None)
def weighted_want(dims):
    free, srcs = search_box(dims)
    cost = np.random.RandomState(7).randint(1, W.COST_MAX + 1, size=free.size).astype(np.uint8)   # 1 .. 8: a ring of 9 slots
    cost.setflags(write=False)
    return cost, W.fields(free, cost, dims, srcs), W.paths(free, cost, dims, *pairs_of(free, srcs))


@pytest.mark.parametrize("dims", SEARCH_DIMS, ids=dims_id)
def test_weighted_in_three_chunks(ctx, dims):
    free, srcs = search_box(dims)
    cost, want, (w_dist, w_len, w_paths) = weighted_want(dims)
    assert (want[:, free != 0] == W.NONE).any() and int(cost[free != 0].max()) == W.COST_MAX
    g = unit_grid(ctx, free, dims)
    with environ(WA_GEO_CHUNK=3), poisoned(ctx):
        assert np.array_equal(g.weighted_fields(cost, srcs), want)
        assert np.array_equal(g.weighted_matrix(cost, srcs), want[:, srcs])
        dist, lens, paths = api.weighted_paths(g, cost, *pairs_of(free, srcs))
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    same_paths(paths, w_paths)
    g.close()


CHAMFER_STEPS = [(3, 4, 5), (1, 16, 16)]


@functools.lru_cache(None)
def chamfer_want(dims, step):
    free, srcs = search_box(dims)
    return CH.fields(free, step, dims, srcs), CH.paths(free, step, dims, *pairs_of(free, srcs))


@pytest.mark.parametrize("step", CHAMFER_STEPS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("dims", SEARCH_DIMS, ids=dims_id)
def test_chamfer_in_three_chunks(ctx, dims, step):
    free, srcs = search_box(dims)
    want, (w_dist, w_len, w_paths) = chamfer_want(dims, step)
    assert (want[:, free != 0] == CH.NONE).any()
    g = unit_grid(ctx, free, dims)
    with environ(WA_GEO_CHUNK=3), poisoned(ctx):
        assert np.array_equal(g.chamfer_fields(step, srcs), want)
        assert np.array_equal(g.chamfer_matrix(step, srcs), want[:, srcs])
        dist, lens, paths = api.chamfer_paths(g, step, *pairs_of(free, srcs))
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    same_paths(paths, w_paths)
    g.close()


@functools.lru_cache(None)
def chamfer_weighted_want(dims):
    free, srcs = search_box(dims)
    step = (3, 4, 5)
    rs = np.random.RandomState(11)
    pen = np.where(rs.uniform(size=free.size) < 0.5, 0, rs.randint(0, CW.PEN_MAX + 1, size=free.size)).astype(np.uint8)
    pen[np.flatnonzero(free)[5]] = CW.PEN_MAX     # penalties up to 31: a ring of 5 + 31 + 1 slots
    pen.setflags(write=False)
    return step, pen, CW.fields(free, step, pen, dims, srcs), CW.paths(free, step, pen, dims, *pairs_of(free, srcs))


@pytest.mark.parametrize("dims", SEARCH_DIMS, ids=dims_id)
def test_chamfer_weighted_in_three_chunks(ctx, dims):
    free, srcs = search_box(dims)
    step, pen, want, (w_dist, w_len, w_paths) = chamfer_weighted_want(dims)
    assert (want[:, free != 0] == CW.NONE).any()
    g = unit_grid(ctx, free, dims)
    with environ(WA_GEO_CHUNK=3), poisoned(ctx):
        assert np.array_equal(g.chamfer_weighted_fields(step, pen, srcs), want)
        assert np.array_equal(g.chamfer_weighted_matrix(step, pen, srcs), want[:, srcs])
        dist, lens, paths = api.chamfer_weighted_paths(g, step, pen, *pairs_of(free, srcs))
    assert np.array_equal(dist, w_dist) and np.array_equal(lens, w_len)
    same_paths(paths, w_paths)
    g.close()


def test_refused_search_calls_leave_the_outputs_untouched(ctx):
    """a source on an occupied voxel: WA_ERR_ARG, and nothing of the poisoned blocks reaches the caller's arrays"""
    dims = (65, 5, 3)
    free, srcs = search_box(dims)
    g = unit_grid(ctx, free, dims)
    bad = np.array([srcs[0], int(np.flatnonzero(free == 0)[0])], np.int64)
    out = np.full((2, free.size), 12345, np.int32)
    cost = np.ones(free.size, np.uint8)
    step = np.array([3, 4, 5], np.int32)
    lib = ctx.lib
    with poisoned(ctx):
        assert lib.wa_grid_geodesic_fields(g.h, bad.ctypes.data, 2, out.ctypes.data) == ARG
        assert lib.wa_grid_weighted_fields(g.h, cost.ctypes.data, bad.ctypes.data, 2, out.ctypes.data) == ARG
        assert lib.wa_grid_chamfer_fields(g.h, step.ctypes.data, bad.ctypes.data, 2, out.ctypes.data) == ARG
        assert lib.wa_grid_chamfer_weighted_fields(g.h, step.ctypes.data, cost.ctypes.data, bad.ctypes.data, 2, out.ctypes.data) == ARG
    assert (out == 12345).all()
    g.close()


# ------------------------------------------------------------------ 3. clearance: distance field, inflation, trajectory check
@functools.lru_cache(None)
def clearance_case(dims):
    """8 % metal, axis tables off the unit lattice; trajectories of 1, 2 and 257 samples on nodes, between them and outside"""
    nx, ny, nz = dims
    rs = np.random.RandomState(nx * 7 + ny)
    free = (rs.uniform(size=nx * ny * nz) >= 0.08).astype(np.uint8)
    free[0] = free[-1] = 1
    axes = tuple((np.arange(k) * s - 1).astype(np.float32) for k, s in zip(dims, (0.25, 0.5, 1.0)))
    d2 = CL.edt_separable(free, nx, ny, nz)
    assert np.array_equal(d2, CL.edt_brute(free, nx, ny, nz))
    keep = np.array([0, nx * ny * nz - 1, int(np.flatnonzero(free)[len(free) // 3])], np.int64)   # bubbles clipped at two corners
    inflated = {r: CL.inflate(free, d2, nx, ny, nz, r, keep) for r in (1.0, 2.5)}
    trajs = []
    for n in (1, 2, 257):
        xyz = np.stack([rs.uniform(axes[c][0] - 0.6, axes[c][-1] + 0.6, n) for c in range(3)], 1).astype(np.float32)
        xyz[::5] = np.stack([axes[c][rs.randint(0, dims[c], len(xyz[::5]))] for c in range(3)], 1)
        trajs.append((xyz, CL.clearance(free, d2, nx, ny, nz, *axes, xyz)))
    return free, axes, d2, keep, inflated, trajs


@pytest.mark.parametrize("dims", [(65, 2, 3), (3, 65, 2)], ids=dims_id)
def test_clearance_on_poisoned_memory(ctx, dims):
    free, axes, d2, keep, inflated, trajs = clearance_case(dims)
    g = api.Grid.from_occupancy(ctx, free, *axes, 1.0, 0)
    for r, want in inflated.items():     # (the first call builds d2)
        with poisoned(ctx):
            gi = g.inflate(r, keep)
        assert np.array_equal(gi.occupancy(), want) and gi.n_free == int(want.sum())
        gi.close()
    assert np.array_equal(g.distance_field(), d2)
    for xyz, (wi, wd, wh, ws) in trajs:
        t = api.Trajectory.from_points(ctx, xyz)
        with poisoned(ctx):
            ids, sd, hit, s = t.clearance(g)
        assert np.array_equal(ids, wi) and np.array_equal(sd, wd) and np.array_equal(hit, wh) and s == ws, (len(xyz), s, ws)
        t.close()
    assert any(ws["n_hit"] > 0 for _, (_, _, _, ws) in trajs) and any(ws["n_outside"] > 0 for _, (_, _, _, ws) in trajs)
    g.close()


def test_refused_inflate_builds_nothing(ctx):
    """a keep id on the metal: refused behind the distance field, which this first call on the grid builds on poisoned blocks"""
    free, axes, d2, keep, inflated, trajs = clearance_case((65, 2, 3))
    g = api.Grid.from_occupancy(ctx, free, *axes, 1.0, 0)
    occ = np.array([int(np.flatnonzero(free == 0)[0])], np.int64)
    h = C.c_void_p(0x1234)
    with poisoned(ctx):
        assert ctx.lib.wa_grid_inflate(g.h, C.c_float(1.0), occ.ctypes.data, 1, C.byref(h)) == ARG
    assert not h.value        # (the call's contract: *out is NULL on every refusal)
    assert np.array_equal(g.distance_field(), d2)
    g.close()


# ------------------------------------------------------------------ 4. line-of-sight shortcuts
@functools.lru_cache(None)
def shortcut_case():
    """65 x 9 x 2: slab z = 0 is a serpentine corridor (a straight stretch can be shortened, a turn cannot), slab z = 1 is open (a snake
    there is shortened across its rows).  Paths of 255, 256 and 257 nodes -- one lane per path, one wavefront per node: a block's edge --
    and of 1 and 2 nodes, which have nothing to shorten."""
    nx, ny, nz = 65, 9, 2
    free = np.concatenate([G.serpentine(nx, ny), np.ones(nx * ny, np.uint8)])
    corridor = []
    for y in range(0, ny, 2):
        xs = range(nx) if (y // 2) % 2 == 0 else range(nx - 1, -1, -1)
        corridor += [vid((nx, ny, nz), x, y, 0) for x in xs]
        if y + 1 < ny:
            corridor.append(vid((nx, ny, nz), xs[-1], y + 1, 0))
    snake = []
    for y in range(ny):
        xs = range(nx) if y % 2 == 0 else range(nx - 1, -1, -1)
        snake += [vid((nx, ny, nz), x, y, 1) for x in xs]
    paths = [np.array(p, np.int64) for p in (corridor[:255], snake[:256], corridor[3:260], snake[100:357], corridor[:1], snake[:2], corridor[60:62])]
    assert all((free[p] != 0).all() for p in paths)
    cx, cy, cz = (np.arange(k, dtype=np.float32) * np.float32(s) for k, s in ((nx, 0.5), (ny, 0.25), (nz, 1.5)))
    import shortcut_ref as S
    want = {}
    for span in (128, 7):
        cache = {}
        want[span] = [S.shortcut(free, nx, ny, cx, cy, cz, p, span, cache) for p in paths]
    return free, (nx, ny, nz), (cx, cy, cz), paths, want


@pytest.mark.parametrize("span", [128, 7])
def test_shortcut_batch_around_a_block(ctx, span):
    free, dims, axes, paths, want = shortcut_case()
    g = api.Grid.from_occupancy(ctx, free, *axes, 1.0, 0)
    with poisoned(ctx):
        wps, lengths = api.shortcut_paths(g, paths, span)
    for p, w, ln, (ww, wl) in zip(paths, wps, lengths, want[span]):
        assert np.array_equal(w, p[ww]) and np.float64(ln).view(np.uint64) == np.float64(wl).view(np.uint64)
    if span == 128:
        assert any(len(ww) < len(p) // 8 for p, (ww, _) in zip(paths, want[span])) and len(want[span][5][0]) == 2
    g.close()


def test_refused_shortcut_leaves_the_outputs_untouched(ctx):
    """(the ids are checked on the host before any device block is allocated: no counter to assert here)"""
    free, dims, axes, paths, want = shortcut_case()
    g = api.Grid.from_occupancy(ctx, free, *axes, 1.0, 0)
    ids = np.concatenate(paths[:2])
    ids[300] = g.n          # outside the grid
    off = np.array([0, 255, 511], np.int64)
    wp, cnt, ln = np.full(511, 777, np.int64), np.full(2, 777, np.int32), np.full(2, 7.0)
    assert ctx.lib.wa_grid_path_shortcut(g.h, ids.ctypes.data, off.ctypes.data, 2, 128, wp.ctypes.data, cnt.ctypes.data, ln.ctypes.data) == ARG
    assert (wp == 777).all() and (cnt == 777).all() and (ln == 7.0).all()
    g.close()


# ------------------------------------------------------------------ 5. seam tours: search, rules, the exact programmes
# (m, closed, or_len, n_starts): M = m or m + 1 from 1 to 34; 63 / 65 starts: fewer and more than a wavefront of them
SEAM_CASES = [(1, True, 3, 1), (1, False, 3, 63), (2, True, 3, 65), (2, False, 2, 1), (17, True, 3, 63), (17, False, 3, 65), (33, True, 3, 65),
              (33, False, 1, 63)]


@functools.lru_cache(None)
def seam_want(case):
    import seamrules_ref as SR
    import seamtour_ref as ST
    from test_gpu_seamrules import kw_rules, rules_of
    from test_gpu_seamtour import euclid
    m, closed, or_len, n_starts = SEAM_CASES[case]
    d = euclid(m, 500 + case)
    kw = dict(closed=closed, or_len=or_len, n_starts=n_starts, seed=0xBEEF + case)
    plain = ST.seam_tour(d, m, **kw)
    # a precedence chain over all seams with the recipe's one-way seams ('t'), and the random recipe ('r')
    ruled = []
    for rk in ("t", "r"):
        b, a, fx = rules_of(rk, m, 70 + case, closed)
        ruled.append(((b, a, fx), SR.seam_tour_rules(d, m, **kw_rules(b, a, fx), **kw)))
    return d, kw, plain, ruled


@pytest.mark.parametrize("case", range(len(SEAM_CASES)))
def test_seam_tours_and_rules(ctx, case):
    from test_gpu_seamtour import same
    d, kw, plain, ruled = seam_want(case)
    with poisoned(ctx, "ctx"):
        got = api.seam_tour(ctx, d, **kw)
    same(got, plain)
    for (b, a, fx), want in ruled:
        with poisoned(ctx, "ctx"):
            got = api.seam_tour_rules(ctx, d, b, a, fx, **kw)
        same(got, want)


@functools.lru_cache(None)
def seam_exact_want(closed):
    import seamrules_ref as SR
    import seamtour_ref as ST
    from test_gpu_seamrules import kw_rules, rules_of
    from test_gpu_seamtour import euclid
    m = 12 if closed else 11      # M = 12 either way
    d = euclid(m, 640 + closed)
    b, a, fx = rules_of("r", m, 41, closed)
    return d, (b, a, fx), ST.seam_tour_exact(d, m, closed), SR.seam_tour_rules_exact(d, m, closed=closed, **kw_rules(b, a, fx))


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
def test_seam_exact_programmes_at_12(ctx, closed):
    d, (b, a, fx), want, want_rules = seam_exact_want(closed)
    with poisoned(ctx, "ctx"):
        got = api.seam_tour_exact(ctx, d, closed)
    assert got["cost_q"] == want["cost_q"] and np.array_equal(got["order"], want["order"]) and np.array_equal(got["dir"], want["dir"])
    with poisoned(ctx, "ctx"):
        got = api.seam_tour_rules_exact(ctx, d, b, a, fx, closed=closed)
    assert got["cost_q"] == want_rules["cost_q"]
    assert np.array_equal(got["order"], want_rules["order"]) and np.array_equal(got["dir"], want_rules["dir"])


# ------------------------------------------------------------------ 6. trajectory fit: leg counts around a block, several rounds
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n_legs", [1, 255, 256, 257])
def test_fit_refines_on_poisoned_memory(ctx, n_legs):
    """fit_ref.many_legs_case: metal under marked polyline points, so the legs around them are blamed, raised and blamed again (level,
    mark, the offsets and the spline's arrays are reused between rounds); the restatement's result is computed once per process"""
    import fit_ref as F
    from test_gpu_fit import _same, grid_of
    scene, par, r = F.many_legs_case(n_legs, 3)
    assert r["rounds"] >= 3 and r["max_level_used"] >= 1      # the first fit and at least two refinement rounds
    with poisoned(ctx):
        g = grid_of(ctx, scene)
        _, out = _same(ctx, scene, *par, grid=g, ref=r)
        out[5].close()       # (the spline: the helper hands it on)
        g.close()


# ------------------------------------------------------------------ 7. torch axes and the check
TORCH_CORNERS = [(1, 33), (65, 64), (256, 64)]


@functools.lru_cache(None)
def torch_case(K, n_beads):
    """97 samples (three tiles of 32 and one sample) over 3 legs in a 32^3 grid of boxes, wishes on two samples of three, both pins"""
    import torch_ref as T
    from test_gpu_torch import _polyline
    grid = T.boxes_grid(np.random.RandomState(7), 32, 8)
    rs = np.random.RandomState(K * 100 + n_beads)
    xyz = _polyline(rs, 32, 97)
    dirs = T.fib_dirs(K, 2.2, (0.2, -0.3, 1.0))
    want = rs.normal(size=(97, 3)).astype(np.float32)
    want[::3] = 0
    off = np.array([0, 33, 34, 97], np.int64)
    pf, pl = rs.randint(-1, K, 3).astype(np.int32), rs.randint(-1, K, 3).astype(np.int32)
    w = T.weights(3, 2, 5, 6, 1 << 17)
    tool = T.rod(n_beads, 16 * 9, 2)
    r = T.plan(grid, xyz, dirs, tool, w, want, off, pf, pl)
    axes = np.asarray(dirs, np.float32).reshape(-1, 3)[r["dir"]]
    return grid, xyz, dirs, tool, w, want, off, pf, pl, r, axes, T.check(grid, xyz, axes, tool, w["near_add"])


@pytest.mark.parametrize("K,n_beads", TORCH_CORNERS)
def test_torch_axes_and_check(ctx, K, n_beads):
    grid, xyz, dirs, tool, w, want, off, pf, pl, r, axes, (cb, cn, cs) = torch_case(K, n_beads)
    free, _, _, ax = grid
    g = api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)
    t = api.Trajectory.from_points(ctx, xyz)
    with poisoned(ctx):
        o = t.torch_axes(g, dirs, tool, want=want, off=off, pin_first=pf, pin_last=pl, **w)
    assert np.array_equal(o["feas"], r["feas"]) and np.array_equal(o["leg_cost"], r["leg_cost"]) and np.array_equal(o["dir"], r["dir"])
    assert o["summary"] == r["summary"], (o["summary"], r["summary"])
    with poisoned(ctx):
        b, nr, s = t.torch_check(g, axes, tool, w["near_add"])
    assert np.array_equal(b, cb) and np.array_equal(nr, cn) and s == cs, (s, cs)
    t.close()
    g.close()


# ------------------------------------------------------------------ 8. retime, stops, ticks
RT_SIZES = [2, 257, 1025]


@functools.lru_cache(None)
def retime_case(n):
    """test_gpu_stops.stopped_path through a 32^3 grid of boxes: stops on the first and the last segment (n = 2: the one segment), a
    per-sample limit, a slow zone near the metal; then the tick axes of the reference's own times, with and without tags"""
    import retime_ref as R
    import stops_ref as S
    import ticks_ref as K
    import torch_ref as T
    from test_gpu_stops import LIM, TICK, stopped_path
    grid = T.boxes_grid(np.random.RandomState(11), 32, 6)
    stops = [0] if n == 2 else [0, n // 2, n - 2]
    xyz, dwell, q = stopped_path(n, stops, [2.0, 0.3, 12.345])
    lim = dict(LIM, v_near=0.8, near_d2=4)
    v_limit = (0.5 + 3.0 * np.random.RandomState(n).uniform(size=n)).astype(np.float32)
    tool = T.rod(9, 16 * 9, 1)
    rs = S.retime_stops(xyz, lim, dwell, v_limit, grid, TICK)
    tags = (np.arange(n - 1) % 3 * (np.arange(n - 1) % 5 > 0)).astype(np.uint8)
    ts = S.tick_axes_stops(xyz, q, rs["time_q"], rs["w_q"], lim["acc"], lim["dec"], TICK, grid, tool, 4, tags)
    ts0 = S.tick_axes_stops(xyz, q, rs["time_q"], rs["w_q"], lim["acc"], lim["dec"], TICK, grid, tool, 4, None)
    # the plain calls on the same samples without their doubled points
    keep = np.concatenate([[True], (np.diff(xyz, axis=0) != 0).any(1)])
    pxyz, pq, pv = xyz[keep], q[keep], v_limit[keep]
    rp = R.retime(pxyz, lim, pv, grid, TICK) if len(pxyz) >= 2 else None
    tp = K.tick_axes(pxyz, pq, rp["time_q"], rp["w_q"], lim["acc"], lim["dec"], TICK, grid, tool, 4) if rp else None
    return grid, xyz, dwell, q, lim, v_limit, tool, tags, rs, (ts, ts0), (pxyz, pq, pv, rp, tp)


@pytest.mark.parametrize("n", RT_SIZES)
def test_retime_stops_and_tick_axes(ctx, n):
    from test_gpu_stops import TICK
    grid, xyz, dwell, q, lim, v_limit, tool, tags, rs, (ts, ts0), (pxyz, pq, pv, rp, tp) = retime_case(n)
    free, _, _, ax = grid
    g = api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)
    t = api.Trajectory.from_points(ctx, xyz)
    kw = dict(a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"])
    with poisoned(ctx):
        time_q, w_q, bound, ticks, s, ss = t.retime_stops(lim["v_max"], lim["acc"], lim["dec"], TICK, dwell=dwell, v_limit=v_limit, **kw)
    assert s == rs["summary"] and ss == rs["stops"], (s, rs["summary"], ss, rs["stops"])
    assert np.array_equal(time_q, rs["time_q"]) and np.array_equal(w_q, rs["w_q"]) and np.array_equal(bound, rs["bound"])
    assert np.array_equal(bits(ticks.points()), bits(rs["ticks"]))
    ticks.close()
    assert ss["n_stops"] == (1 if n == 2 else 3) and (n == 2 or s["n_bound"][3] > 0)
    with poisoned(ctx):      # every optional output: axes, blocked, tags
        axes, blocked, sm, tg, st = t.tick_axes_stops(q, time_q, w_q, lim["acc"], lim["dec"], TICK, seg_tag=tags, grid=g, tool=tool, near_add=4)
    assert sm == ts["summary"] and st == ts["stops"], (sm, ts["summary"], st, ts["stops"])
    assert np.array_equal(bits(axes.points()), bits(ts["axes"])) and np.array_equal(blocked, ts["blocked"]) and np.array_equal(tg, ts["tag"])
    axes.close()
    with poisoned(ctx):      # ... and none of them
        _, b0, sm0, tg0, st0 = t.tick_axes_stops(q, time_q, w_q, lim["acc"], lim["dec"], TICK, grid=g, tool=tool, near_add=4, axes=False, blocked=False)
    assert b0 is None and tg0 is None and sm0 == ts0["summary"] == sm and st0 == ts0["stops"], (sm0, st0, ts0["stops"])
    t.close()
    if rp is not None:
        t = api.Trajectory.from_points(ctx, pxyz)
        with poisoned(ctx):
            time_q, w_q, bound, ticks, s = t.retime(lim["v_max"], lim["acc"], lim["dec"], TICK, v_limit=pv, **kw)
        assert s == rp["summary"], (s, rp["summary"])
        assert np.array_equal(time_q, rp["time_q"]) and np.array_equal(w_q, rp["w_q"]) and np.array_equal(bound, rp["bound"])
        assert np.array_equal(bits(ticks.points()), bits(rp["ticks"]))
        ticks.close()
        with poisoned(ctx):
            axes, blocked, sm = t.tick_axes(pq, time_q, w_q, lim["acc"], lim["dec"], TICK, g, tool, 4)
        assert sm == tp["summary"] and np.array_equal(bits(axes.points()), bits(tp["axes"])) and np.array_equal(blocked, tp["blocked"])
        axes.close()
        with poisoned(ctx):
            a0, b0, sm0 = t.tick_axes(pq, time_q, w_q, lim["acc"], lim["dec"], TICK, g, tool, 4, axes=False, blocked=False)
        assert a0 is None and b0 is None and sm0 == sm
        t.close()
    g.close()


@functools.lru_cache(None)
def smooth_case(max_level):
    import ticks_ref as K
    grid, xyz, q, tool = K.slab_turn_scene()
    off = np.array([0, 40, len(xyz)], np.int64)
    return grid, xyz, q, tool, off, K.smooth(xyz, q, 3.0, max_level, grid, tool, off), K.limits(xyz, q, 2.0, 1.5, 0.05)


@pytest.mark.parametrize("max_level", [3, 8])
def test_smooth_axes_climbs_on_poisoned_memory(ctx, max_level):
    """the slab scene: wide windows around the change of direction are blocked, so samples climb (k_ax_climb's compacted list)"""
    grid, xyz, q, tool, off, r, rl = smooth_case(max_level)
    assert sum(r["summary"]["n_level"][1:]) > 0
    free, _, _, ax = grid
    g = api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)
    t = api.Trajectory.from_points(ctx, xyz)
    with poisoned(ctx):
        o = t.smooth_axes(q, 3.0, max_level, g, tool, off)
    assert o["summary"] == r["summary"], (o["summary"], r["summary"])
    assert np.array_equal(o["q"], r["q"]) and np.array_equal(o["level"], r["level"]) and np.array_equal(o["blocked"], r["blocked"])
    with poisoned(ctx):
        f, s = t.axis_limits(q, 2.0, 1.5, 0.05)
    assert s == rl["summary"] and np.array_equal(bits(f), bits(rl["v_limit"]))
    t.close()
    g.close()


# ------------------------------------------------------------------ 9. reach, fit grids, penalties; the pose searches
POSE_K = [1, 64, 65]


@functools.lru_cache(None)
def pose_scene(K):
    """65 x 7 x 5 with three boxes (rows of 65 voxels: a wavefront and one lane; 35 rows: the last workgroup of four rows is short one),
    K directions in a cone around +z (K = 65: a second mask word with 63 pad bits), a 4-bead rod, a turn limit that bites"""
    import pose_ref as PR
    import torch_ref as T
    nx, ny, nz = 65, 7, 5
    free = np.ones((nz, ny, nx), np.uint8)
    free[0:3, 2:5, 20:24] = 0
    free[2:5, 0:4, 58:63] = 0
    free[0:4, 3:7, 40:43] = 0
    grid = T.make_grid(free, (nx, ny, nz))
    dirs = T.fib_dirs(K, 1.2, (0.0, 0.0, 1.0))
    tool = T.rod(4, 48, 1)
    max_turn = 30000 if K > 1 else 0
    sc = PR.Scene(grid, dirs, tool, max_turn)
    assert K == 1 or (not sc.adj.all() and sc.adj.sum() > K)
    pts = PR.spread_points(grid, 4)
    pins = [K - 1, -1, 0, -1]
    return dict(grid=grid, dirs=dirs, tool=tool, max_turn=max_turn, points=pts, pins=pins), sc


def pose_grid(ctx, c):
    free, _, _, ax = c["grid"]
    return api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)


def check_pose(ctx, g, sc, c, fields, matrix, paths, lead):
    """fields with states from the first two points, the matrix with pins, all pair paths with their pins -- in chunks of 3 sources"""
    from test_gpu_pose import all_pairs, same_paths as same_pose_paths
    pts, pins = c["points"], c["pins"]
    with environ(WA_GEO_CHUNK=3), poisoned(ctx):
        cost, state = fields(*lead, pts[:2], pins[:2], states=True)
        m = matrix(*lead, pts, pins)
        s, e, ps, pe = all_pairs(pts, pins)
        got = paths(*lead, s, e, ps, pe)
    for i in range(2):
        ws, wc = sc.levels(pts[i], pins[i])
        assert np.array_equal(cost[i], wc) and np.array_equal(state[i], ws), i
    assert np.array_equal(m, sc.matrix(pts, pins))
    same_pose_paths(got, sc.paths(s, e, ps, pe), lead[2])


@pytest.mark.parametrize("K", POSE_K)
def test_pose_hops(ctx, K):
    c, sc = pose_scene(K)
    g = pose_grid(ctx, c)
    check_pose(ctx, g, sc, c, g.pose_fields, g.pose_matrix, g.pose_paths, (c["dirs"], c["tool"], c["max_turn"]))
    g.close()


@functools.lru_cache(None)
def pose_weighted_scene(K):
    """hop cost 2, up to four turn bands, penalties up to 15 next to the metal: the longest ring"""
    import pose_weighted_ref as PW
    from test_gpu_pose_weighted import near_pen
    c, sc0 = pose_scene(K)
    bands = (PW.bands_upto(c["dirs"], c["max_turn"], 4) or []) if K > 1 else []
    tc = [0, 1, 3, 6, 9][:len(bands) + 1]
    pen = near_pen(c["grid"], 15)
    return c, api.pose_costs(2, bands, tc, pen), PW.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], PW.Costs(2, bands, tc, pen))


@pytest.mark.parametrize("K", POSE_K)
def test_pose_weighted(ctx, K):
    c, ac, sc = pose_weighted_scene(K)
    g = pose_grid(ctx, c)
    check_pose(ctx, g, sc, c, g.pose_weighted_fields, g.pose_weighted_matrix, g.pose_weighted_paths, (c["dirs"], c["tool"], c["max_turn"], ac))
    g.close()


@functools.lru_cache(None)
def pose_diag_scene(K):
    import pose_diag_ref as PD
    import pose_weighted_ref as PW
    from test_gpu_pose_weighted import near_pen
    c, sc0 = pose_scene(K)
    bands = (PW.bands_upto(c["dirs"], c["max_turn"], 2) or []) if K > 1 else []
    tc = [0, 1, 3][:len(bands) + 1]
    pen = near_pen(c["grid"], 3)
    return c, api.pose_diag_costs((3, 4, 5), bands, tc, pen), PD.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], PD.Costs((3, 4, 5), bands, tc, pen))


@pytest.mark.parametrize("K", POSE_K)
def test_pose_diag(ctx, K):
    c, ac, sc = pose_diag_scene(K)
    g = pose_grid(ctx, c)
    check_pose(ctx, g, sc, c, g.pose_diag_fields, g.pose_diag_matrix, g.pose_diag_paths, (c["dirs"], c["tool"], c["max_turn"], ac))
    g.close()


REACH_CASES = [(65, 63, 1), (130, 65, 64), (65, 130, 64), (130, 65, 1)]     # (K, nx, beads)


@functools.lru_cache(None)
def reach_case(K, nx, n_beads):
    """nx x 5 x 5 with a block of metal at one end: the far end is farther from it than the rod is long (every direction open without a
    gather), the near end is not"""
    import reach_ref as RR
    import torch_ref as T
    free = np.ones((5, 5, nx), np.uint8)
    free[1:4, 1:4, 2:5] = 0
    free[0:2, 3:5, 10:12] = 0
    grid = T.make_grid(free, (nx, 5, 5))
    dirs = T.fib_dirs(K, 2.0, (0.3, 0.1, 1.0))
    tool = T.rod(n_beads, 16 * 6, 1)
    opened = RR.open_dirs(grid, dirs, tool)
    count = opened.sum(1)
    far, near = RR.far_near(grid, tool)
    assert far.any() and near.any()
    keep = [int(np.flatnonzero(np.asarray(grid[0]).ravel())[7])]
    thr = [1, K // 2, K]
    return (grid, dirs, tool, RR.reach(grid, dirs, tool), keep, RR.fit(grid, dirs, tool, max(1, K // 2), keep, 5, count=count), thr,
            RR.penalties(grid, dirs, tool, thr, count=count))


@pytest.mark.parametrize("K,nx,n_beads", REACH_CASES)
def test_reach_fit_penalties(ctx, K, nx, n_beads):
    grid, dirs, tool, (w_mask, w_count, w_sum), keep, w_fit, thr, w_pen = reach_case(K, nx, n_beads)
    free, _, _, ax = grid
    g = api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)
    with poisoned(ctx):
        mask, count, s = g.torch_reach(dirs, tool)
    assert np.array_equal(mask, w_mask) and np.array_equal(count, w_count) and s == w_sum, (s, w_sum)
    with poisoned(ctx):
        gf = g.torch_fit(dirs, tool, max(1, K // 2), keep, 5)
    assert np.array_equal(gf.occupancy(), w_fit) and gf.n_free == int(np.asarray(w_fit).sum()) and gf.reach_summary == w_sum
    gf.close()
    with poisoned(ctx):
        pen = g.torch_penalties(dirs, tool, thr)
    assert np.array_equal(pen, w_pen)
    g.close()


# ------------------------------------------------------------------ 10. trajectory: stitching and B-spline evaluation against the goldens
def test_stitch_and_bspline_goldens(ctx):
    """the golden tour of the cubic demo stitched on a grid voxelised on poisoned memory, and the reference's own spline case
    'd3_full': 300 middle points, 203 parameters and 450 samples -- neither a multiple of 256"""
    import waf
    from test_gpu_trajectory import bits          # (NaNs compare equal whatever their payload: the goldens come from an x86 run)
    from test_trajectory_golden import case, segments_of
    g = waf.load(os.path.join(GOLD, "smooth_cubic_fill0.waf"))
    with poisoned(ctx):
        grid = api.Grid.from_mesh(ctx, api.stl_read_file(os.path.join(GOLD, "cubic.stl")), float("0.0219"), 8)
        ids, off = segments_of(g)
        path = api.Trajectory.stitch(grid, [ids[off[s]:off[s + 1]] for s in range(len(off) - 1)])
    assert np.array_equal(bits(path.points()), bits(np.stack([g["g_path_x"], g["g_path_y"], g["g_path_z"]], axis=1)))
    path.close()
    grid.close()
    c = case("d3_full")
    n, deg = waf.scalar(c, "n_middle"), waf.scalar(c, "deg")
    assert len(c["u"]) % 256 and waf.scalar(c, "count") % 256
    with poisoned(ctx):
        b = api.Bspline(ctx, 3, deg, waf.scalar(c, "ci"), waf.scalar(c, "cf"), n, waf.scalar(c, "fill_bits"))
        b.set_param(c["init"], c["fin"], c["middle"].reshape(n, -1), waf.scalar(c, "tf"))
    knots, cps = b.arrays()
    assert np.array_equal(bits(knots), bits(c["knots"])) and np.array_equal(bits(cps), bits(c["cps"]))
    for d in range(deg + 2):
        with poisoned(ctx):
            out, ok = b.eval(c["u"], d)
        assert np.array_equal(ok, c["ok%d" % d])
        m = ok.astype(bool)
        assert np.array_equal(bits(out[m]), bits(np.asarray(c["der%d" % d]).reshape(len(ok), -1)[m])) and not out[~m].any()
    with poisoned(ctx):
        out, ok = b.sample(waf.scalar(c, "t0"), waf.scalar(c, "dt"), waf.scalar(c, "count"))
    assert ok.all() and np.array_equal(bits(out), bits(c["samples"]))
    b.close()


# ------------------------------------------------------------------ 11. pose shortcut
@functools.lru_cache(None)
def pose_shortcut_case():
    """pose_scene(65)'s grid: a snake over the free voxels of slab z = 4 with the lowest open direction per node, cut into paths of 255,
    256 and 257 nodes (a block's edge for the lane-per-path chain pass), and paths of 1 and 2 nodes"""
    import pose_shortcut_ref as PS
    c, sc0 = pose_scene(65)
    sc = PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], sc0.opened)
    nx, ny, nz = 65, 7, 5
    snake = []
    for y in range(ny):
        xs = range(nx) if y % 2 == 0 else range(nx - 1, -1, -1)
        snake += [vid((nx, ny, nz), x, y, 4) for x in xs]
    snake = np.array([v for v in snake if sc0.opened[v].any()], np.int64)
    assert len(snake) >= 400
    paths = [snake[:255], snake[40:296], snake[100:357], snake[:1], snake[7:9]]
    kss = [PS.lowest_open(sc0.opened, p) for p in paths]
    return c, sc, paths, kss, sc.batch(paths, kss, 24)


def test_pose_shortcut_batch_around_a_block(ctx):
    from test_gpu_pose_shortcut import check
    c, sc, paths, kss, (ww, wh, wl, ws) = pose_shortcut_case()
    assert ws["n_held_start"] > 0 and ws["n_waypoints"] < ws["n_nodes"]
    g = pose_grid(ctx, c)
    with poisoned(ctx):
        check(g, sc, paths, kss, 24, "poisoned")
    g.close()


# ------------------------------------------------------------------ 12. pose fit
@pytest.mark.parametrize("degree", [2, 3])
def test_pose_fit_on_pillars(ctx, degree):
    """pose_fit_ref's pillars scene at 257 samples (256 segments and one sample more than a block): several refinement rounds on the
    buffers of the trajectory fit plus the masks, the holds and the segment directions"""
    import pose_fit_ref as PF
    from test_gpu_pose_fit import grid_of, same
    s = PF.scene("pillars4")
    r = PF.fitted("pillars4", degree, 8.0, 6, 257)
    assert r["rounds"] >= 3
    g = grid_of(ctx, s["grid"])
    with poisoned(ctx):
        same(ctx, g, r, s["xyz"], s["dirs"], s["tool"], s["holds"], degree, 8.0, 6, 257, ("poisoned pillars4", degree))
    g.close()


# ------------------------------------------------------------------ 13. pose fit at leg counts around a block
@functools.lru_cache(None)
def pose_fit_legs_case(n_legs):
    """fit_ref.many_legs_scene (metal under marked polyline points: the legs around them are blamed until they reach the cap) with three
    directions, a two-bead rod and a hold per leg that runs through -1, 0, 1, 2"""
    import fit_ref as F
    import pose_fit_ref as PF
    import torch_ref as T
    free, d2, dims, axes, xyz = F.many_legs_scene(n_legs, F.block_marks(n_legs), n_legs)
    grid = (free, d2, dims, axes)
    dirs = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float32)
    tool = T.rod(2, 32, 0)
    holds = (np.arange(n_legs) % 4 - 1).astype(np.int32)
    return grid, dirs, tool, xyz, holds, PF.fit(grid, dirs, tool, xyz, holds, 3, 1.0, 2, F.BLOCK_SAMPLES)


@pytest.mark.parametrize("n_legs", [1, 255, 256, 257])
def test_pose_fit_leg_counts_around_the_block(ctx, n_legs):
    import fit_ref as F
    from test_gpu_pose_fit import grid_of, same
    grid, dirs, tool, xyz, holds, r = pose_fit_legs_case(n_legs)
    assert r["rounds"] >= 3
    g = grid_of(ctx, grid)
    with poisoned(ctx):
        same(ctx, g, r, xyz, dirs, tool, holds, 3, 1.0, 2, F.BLOCK_SAMPLES, ("poisoned legs", n_legs))
    g.close()


# ------------------------------------------------------------------ 14. the ACS-TSP on every kernel the dispatch can select
GTSP_SMALLEST = {"wave8": 2, "wave16": 129, "fast1": 2, "fast2": 65, "fast4": 129, "generic_forced": 2, "generic": 257}


@functools.lru_cache(None)
def gtsp_case(variant, sizes=None):
    """the variant's smallest size of tests/test_gpu_gtsp_dispatch.py (and 9 cities for the kernels that start at 2: a tour with a
    choice in it) unless sizes are given, the oracle's answers in DEV and in REF mode"""
    import oracle_lib as O
    from test_gpu_gtsp_dispatch import cap, points
    out = []
    for n in sizes or sorted({GTSP_SMALLEST[variant], max(GTSP_SMALLEST[variant], 9)}):
        d = points(np.random.RandomState(n + len(variant)), n)
        dev = O.gtsp_solve(d, mode=O.DEV, seed=1000 + n, stream=n, max_iterations=cap(n), want_pher=True)
        rng = O.srand(77)
        st = np.array(list(rng.r) + [rng.f, rng.b], np.int32)
        ref = O.gtsp_solve(d, mode=O.REF, rng=rng, max_iterations=cap(n), want_pher=True)
        out.append((n, d, dev, st, ref, (list(rng.r)[:31], rng.f, rng.b)))
    return out


@pytest.mark.parametrize("variant", list(GTSP_SMALLEST))
def test_gtsp_dispatch_on_poisoned_memory(ctx, variant):
    from test_gpu_gtsp_dispatch import VARIANTS
    assert GTSP_SMALLEST[variant] == min(VARIANTS[variant][1])
    run_gtsp(ctx, variant, gtsp_case(variant))


def run_gtsp(ctx, variant, cases):
    from test_gpu_gtsp_dispatch import KERNEL, VARIANTS, cap, check, dispatch
    kn, sizes = VARIANTS[variant]
    env = {}
    if kn.get("wave") is not None:
        env["WA_GTSP_WAVE"] = 1 if kn["wave"] else 0
    if kn.get("generic"):
        env["WA_GTSP_GENERIC"] = 1
    for n, d, dev, st, ref, (rr, rf, rb) in cases:
        assert dispatch(n, 1, **kn) == KERNEL[variant]
        with environ(WA_GTSP_WAVE="", WA_GTSP_GENERIC=""), environ(**env), poisoned(ctx):
            t = api.gtsp_solve(ctx, d, mode=api.RNG_DEV, seed=1000 + n, stream=n, max_iterations=cap(n), want_pher=True)
            u = api.gtsp_solve(ctx, d, mode=api.RNG_REF, rand_state=st.copy(), max_iterations=cap(n), want_pher=True)
        check(t, 0, dev, (variant, n, "dev"))
        check(u, 0, ref, (variant, n, "ref"))
        assert [int(v) for v in u["rand_state"][:31]] == rr and (int(u["rand_state"][34]), int(u["rand_state"][35])) == (rf, rb)


# ------------------------------------------------------------------ 15. refused calls of the trajectory stages and the seam tours
def test_refused_trajectory_calls_copy_no_poison_to_the_host(ctx):
    """A coordinate that is not finite is found by the kernels, so each call below has allocated its poisoned blocks and run on them
    before it answers WA_ERR_ARG: the caller's arrays, handles and summaries keep their sentinels.  One refused call per family:
    torch axes and check, fit, pose fit, retime, stops, smoothing and tick axes."""
    import torch_ref as T
    from test_gpu_pose_fit import raw as pose_fit_raw, untouched as pose_fit_untouched
    from welding_robot_amd import _lib as L
    lib = ctx.lib
    grid = T.boxes_grid(np.random.RandomState(7), 32, 8)
    free, _, _, ax = grid
    g = api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)
    n, K = 40, 8
    xyz = np.stack([np.linspace(3, 28, n), np.linspace(4, 27, n), np.full(n, 16.0)], 1).astype(np.float32)
    xyz[7, 1] = np.nan
    t = api.Trajectory.from_points(ctx, xyz)
    dirs = np.ascontiguousarray(T.fib_dirs(K, 1.0), np.float32)
    tool = api.torch_tool(*T.rod(3, 48, 1))
    P = lambda a: a.ctypes.data   # noqa: E731
    # torch axes / check
    w = L.ToolWeights(1, 0, 1, -1, -1)
    off = np.array([0, n], np.int64)
    dir_out, feas, cost = np.full(n, -7, np.int32), np.full((n, K), 77, np.uint8), np.full(1, -7, np.int64)
    s = L.ToolSummary()
    s.n = -7
    with poisoned(ctx):
        assert lib.wa_traj_tool_axes(g.h, t.h, P(dirs), K, C.byref(tool), C.byref(w), None, P(off), 1, None, None, P(dir_out), P(feas), P(cost),
                                     C.byref(s)) == ARG
    assert (dir_out == -7).all() and (feas == 77).all() and (cost == -7).all() and s.n == -7
    axes = np.tile(np.float32([0, 0, 1]), (n, 1))
    bl, nr = np.full(n, 77, np.uint8), np.full(n, 77, np.uint8)
    with poisoned(ctx):
        assert lib.wa_traj_tool_check(g.h, t.h, P(axes), C.byref(tool), -1, P(bl), P(nr), C.byref(s)) == ARG
    assert (bl == 77).all() and (nr == 77).all() and s.n == -7
    # fit
    lv = np.full(n + 1, -7, np.int32)
    bh, th, fs = C.c_void_p(0x1234), C.c_void_p(0x5678), L.FitSummary()
    fs.rounds = -9
    with poisoned(ctx):
        assert lib.wa_grid_fit_trajectory(g.h, t.h, 3, C.c_float(8.0), 6, 601, P(lv), C.byref(bh), C.byref(th), C.byref(fs)) == ARG
    assert (lv == -7).all() and bh.value == 0x1234 and th.value == 0x5678 and fs.rounds == -9
    # pose fit
    with poisoned(ctx):
        o = pose_fit_raw(g, t, dirs, tool, np.zeros(n - 1, np.int32), n_samples=601)
    assert o["rc"] == ARG and pose_fit_untouched(o)
    # retime, retime with stops
    lim = L.RetimeLimits(1.0, 1.0, 1.0, float("inf"), 0.5, 4)
    tq, wq, bd = np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(n, 0xAB, np.uint8)
    hh, rs = C.c_void_p(4242), L.RetimeSummary()
    rs.n = -7
    with poisoned(ctx):
        assert lib.wa_traj_retime(g.h, t.h, C.byref(lim), None, C.c_double(0.01), P(tq), P(wq), P(bd), C.byref(hh), C.byref(rs)) == ARG
    assert (tq == -7).all() and (wq == -7).all() and (bd == 0xAB).all() and hh.value == 4242 and rs.n == -7
    dwell = np.full(n - 1, -1.0)
    ss = L.StopsSummary()
    ss.n_stops = -7
    with poisoned(ctx):
        assert lib.wa_traj_retime_stops(g.h, t.h, C.byref(lim), None, P(dwell), C.c_double(0.01), P(tq), P(wq), P(bd), C.byref(hh), C.byref(rs),
                                        C.byref(ss)) == ARG
    assert (tq == -7).all() and (wq == -7).all() and (bd == 0xAB).all() and hh.value == 4242 and rs.n == -7 and ss.n_stops == -7
    # smoothing and tick axes
    q = np.tile(np.int32([0, 0, 16384]), (n, 1))
    qo, lvl, blk = np.full((n, 3), 77, np.int32), np.full(n, 77, np.uint8), np.full(n, 77, np.uint8)
    sm = L.AxesSmoothSummary()
    sm.n = -5
    with poisoned(ctx):
        assert lib.wa_traj_axes_smooth(g.h, t.h, P(q), C.byref(tool), P(off), 1, C.c_double(1.0), 3, P(qo), P(lvl), P(blk), C.byref(sm)) == ARG
    assert (qo == 77).all() and (lvl == 77).all() and (blk == 77).all() and sm.n == -5
    time_q = (np.arange(n, dtype=np.int64) * (1 << 26))
    w_q = np.full(n, 1 << 28, np.int64)
    n_ticks = int(time_q[-1]) // (1 << 20) + 2
    tb, ah, ts = np.full(n_ticks, 77, np.uint8), C.c_void_p(4242), L.TickAxesSummary()
    ts.n_ticks = -5
    with poisoned(ctx):
        assert lib.wa_traj_tick_axes(g.h, t.h, P(q), C.byref(tool), -1, C.c_double(1.0), C.c_double(1.0), C.c_double(2.0 ** -10), P(time_q), P(w_q),
                                     C.byref(ah), P(tb), C.byref(ts)) == ARG
    assert (tb == 77).all() and ah.value == 4242 and ts.n_ticks == -5
    tg, st2 = np.full(n_ticks, 77, np.uint8), L.TickStopsSummary()
    st2.n_tagged = -5
    seg_tag = np.ones(n - 1, np.uint8)
    with poisoned(ctx):
        assert lib.wa_traj_tick_axes_stops(g.h, t.h, P(q), C.byref(tool), -1, C.c_double(1.0), C.c_double(1.0), C.c_double(2.0 ** -10), P(time_q),
                                           P(w_q), P(seg_tag), C.byref(ah), P(tb), P(tg), C.byref(ts), C.byref(st2)) == ARG
    assert (tb == 77).all() and (tg == 77).all() and ah.value == 4242 and ts.n_ticks == -5 and st2.n_tagged == -5
    t.close()
    g.close()


def test_refused_seam_tours_leave_the_outputs_untouched(ctx):
    """(every refusal of the seam tours is decided on the host before a device block is allocated -- the cost matrix, the parameters, the
    start and the rules are host arrays: there is no counter to assert; the sentinels say that nothing was written)"""
    from test_gpu_seamtour import euclid
    from welding_robot_amd import _lib as L
    lib = ctx.lib
    m = 6
    dist = np.ascontiguousarray(euclid(m, 1), np.float64)
    bad = dist.copy()
    bad[0, 3] = bad[3, 0] = np.nan          # (between two seams: an entry the quantisation reads)
    p = L.SeamParams(1, 3, 4, 100, 5)
    P = lambda a: a.ctypes.data   # noqa: E731
    order, dirs = np.full(16, -7, np.int32), np.full(16, 9, np.uint8)
    costs, passes = np.full(8, -7, np.int64), np.full(8, -7, np.int32)
    s, sr = L.SeamSummary(), L.SeamRulesSummary()
    s.cost_q = sr.cost_q = -7
    assert lib.wa_gtsp_seam_tour(ctx.h, P(bad), m, C.byref(p), None, None, P(order), P(dirs), P(costs), P(passes), C.byref(s)) == ARG
    cyc_b, cyc_a = np.array([1, 2], np.int32), np.array([2, 1], np.int32)     # seam 1 before 2 before 1: no admissible order
    assert lib.wa_gtsp_seam_tour_rules(ctx.h, P(dist), m, C.byref(p), P(cyc_b), P(cyc_a), 2, None, None, None, P(order), P(dirs), P(costs),
                                       P(passes), C.byref(sr)) == ARG
    cq = C.c_int64(-7)
    assert lib.wa_gtsp_seam_tour_exact(ctx.h, P(bad), m, 1, P(order), P(dirs), C.byref(cq)) == ARG
    assert lib.wa_gtsp_seam_tour_rules_exact(ctx.h, P(dist), m, 1, P(cyc_b), P(cyc_a), 2, None, P(order), P(dirs), C.byref(cq)) == ARG
    assert (order == -7).all() and (dirs == 9).all() and (costs == -7).all() and (passes == -7).all()
    assert s.cost_q == -7 and sr.cost_q == -7 and cq.value == -7
