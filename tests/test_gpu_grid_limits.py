"""The largest grids the library accepts, on the GPU and against the oracle.

tests/test_grid_limit_rules.py reads the limits back from the source; this file takes its sizes from there.

  creation   wa_grid_from_occupancy at 2^29 and 2^29 + 1 voxels, the 6-neighbour solver (dense and lazy) at 89,478,485 and one
             more, the 26-neighbour solver (dense and lazy) at 2^27 and one more: accepted means a usable handle, refused WA_ERR_ARG.
  6 nb top   n = 89,478,485 exactly: the walk's 32-bit byte offsets (24 B per voxel) reach 2^31 - 8.  One search ends
             at id n - 1 in the top slab; one starts at id 0 and climbs to the top slab (negative neighbour offsets clamped at the
             bottom).  Every launch variant the solver has -- hand-scheduled loop with and without look-ahead, compiler-scheduled loop,
             16-bit tabu entries with the full 12-bit quotient (27-bit ids), tables too small for them, bitmap spills, lazy fields, a
             3-search lazy batch, REF mode -- must equal the same oracle run.  25- and 26-bit grids with 16-bit entries at the
             smallest table that can name their ids.
  26 nb      both sides of the fast loop's bound (104 B records below 2^31 bytes: n <= 20,648,881), dense and lazy, and 2^27 voxels,
             where only the general loop (64-bit offsets) may run, with walks near id 2^27 - 1.

Each comparison is bit for bit: per-generation trace, last generation's ants, best cost and path, and the whole pheromone field
(as digests of 64 MB chunks: tests/limit_ref.py).  Oracle runs go to a pool of spawned workers that import numpy and oracle_lib only."""
import concurrent.futures as cf
import multiprocessing as mp
import os

import numpy as np
import pytest

import limit_ref as R
import oracle_lib as O
from test_grid_limit_rules import DIMS, GRID_MAX, NB6_MAX, NB26_FAST_EDGE, NB26_MAX, SIZES, entries16, id_bits, nb26_fast_loop, \
    smallest_table16
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

SEED, COLONY, OCC = 7, 8, 0.10
GENS6, GENS26, GENS26_MAX = 6, 5, 3


# ------------------------------------------------------------------ grids and searches
def vid(dims, x, y, z):
    nx, ny, _ = dims
    return (z * ny + y) * nx + x


def top_grid(dims, seed, extra=()):
    """a seeded box grid and its searches near the top: `end_last` (30 + 40 voxels from the last id to id n - 1, top slab),
    `climb` (id 0 to the top slab), `mid` (inside the top two slabs)"""
    nx, ny, nz = dims
    s = dict(end_last=(vid(dims, nx - 31, ny - 41, nz - 1), vid(dims, nx - 1, ny - 1, nz - 1)),
             climb=(0, vid(dims, 20, 15, nz - 1)),
             mid=(vid(dims, nx // 2, ny // 2, nz - 1), vid(dims, nx // 2 + 40, ny // 2 + 50, nz - 2)))
    s = {k: v for k, v in s.items() if k in ("end_last",) + tuple(extra)}
    opens = tuple(sorted({v for ab in s.values() for v in ab}))
    return (tuple(dims), seed, OCC, opens), s


SPEC6, SEARCH6 = top_grid(DIMS["nb6_max"], 11, ("climb", "mid"))
STREAM = {"end_last": 0, "climb": 1, "mid": 2}
SPEC25, SEARCH25 = top_grid((256, 256, 257), 12)                 # 16,842,752 voxels: 25-bit ids
SPEC26, SEARCH26 = top_grid((512, 256, 257), 13)                 # 33,685,504 voxels: 26-bit ids
SPEC_FAST, SEARCH_FAST = top_grid(DIMS["nb26_fast"], 14)
SPEC_GEN, SEARCH_GEN = top_grid(DIMS["nb26_general"], 15)
SPEC_MAX26, SEARCH_MAX26 = top_grid(DIMS["nb26_max"], 16)


def task(spec, search, name, nb=6, gens=GENS6, mode="dev"):
    a, b = search[name]
    return (spec, a, b, gens, COLONY, SEED, STREAM[name], nb, mode)


# ------------------------------------------------------------------ oracle pool
class Oracle:
    """oracle runs by task (limit_ref.run_one), cached for the module; computed in spawned workers"""

    def __init__(self):
        O.lib()
        self.pool = cf.ProcessPoolExecutor(max_workers=4, mp_context=mp.get_context("spawn"))
        self.cache = {}

    def prefetch(self, tasks):
        for t in tasks:
            if t not in self.cache:
                self.cache[t] = self.pool.submit(R.run_one, t)

    def get(self, t):
        self.prefetch([t])
        v = self.cache[t]
        if isinstance(v, cf.Future):
            v = self.cache[t] = v.result()
        return v

    def close(self):
        self.pool.shutdown(cancel_futures=True)


SMALL_TASKS = [task(SPEC6, SEARCH6, k) for k in ("end_last", "climb", "mid")] + [task(SPEC6, SEARCH6, "end_last", mode="ref")] + \
    [task(SPEC25, SEARCH25, "end_last"), task(SPEC26, SEARCH26, "end_last")] + \
    [task(s, q, "end_last", nb=26, gens=GENS26) for s, q in ((SPEC_FAST, SEARCH_FAST), (SPEC_GEN, SEARCH_GEN))]


@pytest.fixture(scope="module")
def ref():
    r = Oracle()
    r.prefetch(SMALL_TASKS)
    yield r
    r.close()


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


_dgrids = {}


@pytest.fixture(scope="module")
def grids(ctx):
    """device grids by spec (built once, the largest kept only while their tests run)"""
    yield _dgrids
    for g in _dgrids.values():
        g.close()
    _dgrids.clear()


def dgrid(ctx, spec):
    if spec not in _dgrids:
        g = R.grid(spec)
        _dgrids[spec] = api.Grid.from_occupancy(ctx, g.free, g.cx, g.cy, g.cz, g.precision, g.wall)
    return _dgrids[spec]


def drop(spec):
    g = _dgrids.pop(spec, None)
    if g is not None:
        g.close()


class env:
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def params(gens, mode="dev"):
    if mode == "dev":
        return api.default_params(max_iteration=gens, predict=COLONY / 0.35, fixed_colony=COLONY, rng_mode=api.RNG_DEV, seed=SEED)
    return api.default_params(max_iteration=gens, predict=COLONY / 0.35, fixed_colony=COLONY, rng_mode=api.RNG_REF)


def check(s, q, want, gens, tag):
    t = s.trace(q)
    L, lens = s.ants(q)
    cost, path, _ = s.result(q)
    got = dict(steps=t["steps"][:gens], finite=t["finite"][:gens], bestL=R.bits(t["bestL"][:gens]), colony=t["colony"][:gens],
               antL=R.bits(L), antlen=lens, cost=R.bits(cost), path=path)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), (tag, q, k, v[:8], want[k][:8])
    field = s.pheromone(q)
    got_f = R.field_digests(field)
    del field
    bad = [i for i, (a, b) in enumerate(zip(got_f, want["field"])) if a != b]
    assert len(got_f) == len(want["field"]) and not bad, (tag, q, "field chunks differ", bad[:8], len(got_f))


def solve_and_check(ctx, ref, spec, search, names, nb=6, gens=GENS6, lazy=False, mode="dev", knobs=None):
    """one solver on the grid; the searches one after another (the field re-initialised in between), each against its oracle run"""
    with env(**(knobs or {})):
        s = api.AcsSolver(ctx, dgrid(ctx, spec), n_slots=1, max_colony=COLONY, neighbourhood=nb, lazy=lazy)
    info = []
    try:
        for i, name in enumerate(names):
            if i:
                s.init_pheromone(1.0)
            a, b = search[name]
            if mode == "ref":
                s.srand(SEED)
            s.solve(params(gens, mode), a, b, streams=[STREAM[name]])
            check(s, 0, ref.get(task(spec, search, name, nb=nb, gens=gens, mode=mode)), gens, (name, lazy, mode, knobs))
            if mode == "dev":
                info.append(s.walk_info())
    finally:
        s.close()
    return info


# ------------------------------------------------------------------ creation at every limit and one voxel past it
def refused(fn):
    with pytest.raises(api.WeldacsError) as e:
        fn()
    assert e.value.code == 1, e.value


def ones_grid(ctx, dims):
    free = np.ones(int(np.prod(dims, dtype=np.int64)), np.uint8)
    ax = [np.arange(d, dtype=np.float32) for d in dims]
    return api.Grid.from_occupancy(ctx, free, ax[0], ax[1], ax[2], 1.0, 0)


def test_grid_creation_at_2_pow_29_and_one_more(ctx, ref):
    """(asks for the oracle pool first: its runs go on while the GPU cases before them do)"""
    assert SIZES["grid_max"] == GRID_MAX == 2 ** 29
    g = ones_grid(ctx, DIMS["grid_max"])
    assert (g.nx, g.ny, g.nz) == DIMS["grid_max"] and g.n_free == GRID_MAX       # (the free count runs over every voxel)
    g.close()
    refused(lambda: ones_grid(ctx, DIMS["grid_over"]))


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
def test_6_neighbour_solver_creation_at_the_limit_and_one_more(ctx, grids, lazy):
    g = dgrid(ctx, SPEC6)
    assert g.n == NB6_MAX
    s = api.AcsSolver(ctx, g, n_slots=1, max_colony=COLONY, lazy=lazy)
    s.init_pheromone(1.0)
    s.close()
    over = ones_grid(ctx, DIMS["nb6_over"])
    refused(lambda: api.AcsSolver(ctx, over, n_slots=1, max_colony=COLONY, lazy=lazy))
    over.close()


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
def test_26_neighbour_solver_creation_at_the_limit_and_one_more(ctx, grids, lazy):
    g = dgrid(ctx, SPEC_MAX26)
    assert g.n == NB26_MAX
    s = api.AcsSolver(ctx, g, n_slots=1, max_colony=COLONY, neighbourhood=26, lazy=lazy)
    s.init_pheromone(1.0)
    s.close()
    ctx.trim()
    over = ones_grid(ctx, DIMS["nb26_over"])
    refused(lambda: api.AcsSolver(ctx, over, n_slots=1, max_colony=COLONY, neighbourhood=26, lazy=lazy))
    over.close()


# ------------------------------------------------------------------ 6 neighbours at n = 89,478,485
VARIANTS6 = {
    "default": {},
    "direct": dict(WA_WALK_DIRECT=1),
    "no_lookahead": dict(WA_WALK_WARM=0, WA_WALK_DIRECT=0),
    "compiler_loop": dict(WA_WALK_ASM=0),
    "entries16_q12": dict(WA_TAB16=1, WA_HASH_LOG2=15),
    "entries16_too_narrow": dict(WA_TAB16=1, WA_HASH_LOG2=14),
    "spill": dict(WA_HASH_LOG2=6),        # 48 keys before the bitmap; every walk is longer (70 and 160 lattice steps at the least)
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("variant", sorted(VARIANTS6))
def test_6_neighbours_at_the_top_dense(ctx, grids, ref, variant):
    assert 2 ** 31 - 24 * NB6_MAX == 8                                          # (the last record ends 8 bytes short of 2^31)
    info = solve_and_check(ctx, ref, SPEC6, SEARCH6, ("end_last", "climb"), knobs=VARIANTS6[variant])
    if variant.startswith("entries16"):
        lg = VARIANTS6[variant]["WA_HASH_LOG2"]
        assert all(i["entries16"] == entries16(NB6_MAX, lg) and i["hash_log2"] == lg for i in info), info
        assert id_bits(NB6_MAX) == 27 and entries16(NB6_MAX, 15) and not entries16(NB6_MAX, 14)


@pytest.mark.timeout(900)
def test_6_neighbours_at_the_top_lazy(ctx, grids, ref):
    solve_and_check(ctx, ref, SPEC6, SEARCH6, ("end_last", "climb"), lazy=True)


@pytest.mark.timeout(900)
def test_6_neighbours_at_the_top_lazy_batch_of_three(ctx, grids, ref):
    names = ("end_last", "climb", "mid")
    s = api.AcsSolver(ctx, dgrid(ctx, SPEC6), n_slots=3, max_colony=COLONY, lazy=True)
    try:
        s.solve(params(GENS6), [SEARCH6[k][0] for k in names], [SEARCH6[k][1] for k in names], streams=[STREAM[k] for k in names])
        for q, k in enumerate(names):
            check(s, q, ref.get(task(SPEC6, SEARCH6, k)), GENS6, ("batch", k))
    finally:
        s.close()


@pytest.mark.timeout(900)
def test_6_neighbours_at_the_top_ref_mode(ctx, grids, ref):
    solve_and_check(ctx, ref, SPEC6, SEARCH6, ("end_last",), mode="ref")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("spec,search", [(SPEC25, SEARCH25), (SPEC26, SEARCH26)], ids=["25bit", "26bit"])
def test_entries16_at_the_smallest_table_that_names_the_ids(ctx, grids, ref, spec, search):
    n = int(np.prod(spec[0]))
    lg = smallest_table16(n)
    assert id_bits(n) == lg + 12 and entries16(n, lg) and not entries16(n, lg - 1)
    drop(SPEC6)
    info = solve_and_check(ctx, ref, spec, search, ("end_last",), knobs=dict(WA_TAB16=1, WA_HASH_LOG2=lg))
    assert info[0]["entries16"] and info[0]["hash_log2"] == lg, info
    drop(spec)


# ------------------------------------------------------------------ 26 neighbours around the fast loop's bound, and at 2^27
@pytest.mark.timeout(900)
@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
@pytest.mark.parametrize("side", ["fast", "general"])
def test_26_neighbours_on_both_sides_of_the_fast_loop_bound(ctx, grids, ref, side, lazy):
    spec, search = (SPEC_FAST, SEARCH_FAST) if side == "fast" else (SPEC_GEN, SEARCH_GEN)
    n = int(np.prod(spec[0]))
    assert n == (NB26_FAST_EDGE - 1 if side == "fast" else NB26_FAST_EDGE + 1) and nb26_fast_loop(n) == (side == "fast")
    solve_and_check(ctx, ref, spec, search, ("end_last",), nb=26, gens=GENS26, lazy=lazy)


@pytest.mark.timeout(900)
def test_26_neighbours_at_2_pow_27(ctx, grids, ref):
    """512^3: ids up to 2^27 - 1 fill the path word's id field; the field is 14 GB, the walk's records lie up to 14 GB from its base"""
    for spec in (SPEC_FAST, SPEC_GEN):
        drop(spec)
    t = task(SPEC_MAX26, SEARCH_MAX26, "end_last", nb=26, gens=GENS26_MAX)
    ref.prefetch([t])
    assert not nb26_fast_loop(NB26_MAX) and SEARCH_MAX26["end_last"][1] == NB26_MAX - 1
    solve_and_check(ctx, ref, SPEC_MAX26, SEARCH_MAX26, ("end_last",), nb=26, gens=GENS26_MAX)
    drop(SPEC_MAX26)
