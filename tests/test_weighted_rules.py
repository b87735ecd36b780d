"""CPU checks of the restatement the GPU tests of the weighted shortest paths rely on (tests/weighted_ref.py), and of the Python surface:
hand-made cases written out here, the restatement against scipy's Dijkstra, all-ones costs against the hop restatement, the checker
against doctored fields, the clearance-cost rule against a brute-force count, and the level scheme of the kernel (a ring of W + 1
frontiers, costs paid on entry) restated on boolean arrays against the heap."""
import numpy as np
import pytest

import clearance_ref as CR
import geodesic_ref as G
import weighted_ref as W


def random_case(rs, max_side=8, max_cost=8):
    dims = tuple(int(v) for v in rs.randint(1, max_side + 1, size=3))
    n = int(np.prod(dims))
    free = (rs.uniform(size=n) >= rs.uniform(0.0, 0.4)).astype(np.uint8)
    free[int(rs.randint(n))] = 1
    cost = rs.randint(1, int(rs.randint(1, max_cost + 1)) + 1, size=n).astype(np.uint8)
    return free, cost, dims


def test_the_wrappers_exist():
    from welding_robot_amd import _lib, api
    assert api.WA_COST_MAX == 8 and api.WA_DIST_NONE == -1 == W.NONE and W.COST_MAX == 8
    for name in ("wa_grid_clearance_costs", "wa_grid_weighted_fields", "wa_grid_weighted_matrix", "wa_grid_weighted_paths"):
        assert name in _lib.SYMBOLS
    for name in ("clearance_costs", "weighted_fields", "weighted_matrix"):
        assert callable(getattr(api.Grid, name))
    assert callable(api.weighted_paths)


@pytest.mark.parametrize("case", W.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, free, cost, dims, src, want, want_paths = case
    d = W.field(free, cost, dims, src)
    for v, k in want.items():
        assert d[v] == k, (v, int(d[v]), k)
    for e, p in want_paths.items():
        assert W.walk_back(d, cost, dims, e).tolist() == p
        assert W.path_cost(cost, p) == d[e]
    assert W.locally_exact(d, free, cost, dims, src)


def test_detour_is_longer_and_cheaper():
    _, free, cost, dims, src, _, _ = W.hand_cases()[1]
    d, n, p = W.paths(free, cost, dims, [0], [4])
    hops = G.field(free, dims, 0)[4]
    assert (int(d[0]), int(n[0]), int(hops)) == (6, 7, 4), "6 steps at cost 6 where the 4 hops would cost 11"


def test_tie_is_decided_by_the_neighbour_order():
    free, cost, dims, s, e, want = W.tie_case()
    d = W.field(free, cost, dims, s)
    assert d.tolist() == [0, 1, 2, 1, 3, 3, 2, 3, 4]
    assert W.walk_back(d, cost, dims, e).tolist() == want
    assert W.walk_back(d, cost, dims, s).tolist() == [0]


def test_asymmetry_identity():
    rs = np.random.RandomState(11)
    seen = 0
    for _ in range(40):
        free, cost, dims = random_case(rs)
        pts = np.flatnonzero(free)[:6]
        m = W.matrix(free, cost, dims, pts)
        c = cost[pts].astype(np.int64)
        for i in range(len(pts)):
            for j in range(len(pts)):
                assert (m[i, j] < 0) == (m[j, i] < 0)
                if m[i, j] >= 0:
                    assert m[i, j] - m[j, i] == c[j] - c[i]
                    seen += m[i, j] != m[j, i]
    assert seen > 20, "the cases must hold pairs that differ by direction"


def test_restatement_against_scipy():
    rs = np.random.RandomState(5)
    for k in range(60):
        free, cost, dims = random_case(rs)
        srcs = np.flatnonzero(free)[rs.randint(int(free.sum()), size=3)]
        assert np.array_equal(W.fields(free, cost, dims, srcs), W.scipy_fields(free, cost, dims, srcs)), (k, dims)
    # a larger box with pockets
    dims = (23, 17, 9)
    n = int(np.prod(dims))
    free = (rs.uniform(size=n) >= 0.42).astype(np.uint8)
    free[0] = 1
    cost = rs.randint(1, 9, size=n).astype(np.uint8)
    d = W.field(free, cost, dims, 0)
    assert np.array_equal(d, W.scipy_fields(free, cost, dims, [0])[0])
    assert ((d < 0) & (free != 0)).sum() > 10 and W.locally_exact(d, free, cost, dims, 0)


def test_all_ones_is_the_hop_field():
    rs = np.random.RandomState(2)
    for _ in range(25):
        free, _, dims = random_case(rs)
        ones = np.ones(free.size, np.uint8)
        cand = np.flatnonzero(free)
        s = int(cand[rs.randint(len(cand))])
        d = W.field(free, ones, dims, s)
        assert np.array_equal(d, G.field(free, dims, s))
        ends = cand[rs.randint(len(cand), size=4)]
        wd, wn, wp = W.paths(free, ones, dims, [s] * 4, ends)
        gh, gp = G.paths(free, dims, [s] * 4, ends)
        assert np.array_equal(wd, gh) and np.array_equal(wn, np.maximum(gh + 1, 0))
        for a, b in zip(wp, gp):
            assert (a is None and b is None) or np.array_equal(a, b)


def test_checker_rejects_doctored_fields():
    rs = np.random.RandomState(8)
    dims = (9, 8, 70)       # (more than two slabs of the checker in z)
    n = int(np.prod(dims))
    free = (rs.uniform(size=n) >= 0.25).astype(np.uint8)
    src = 5
    free[src] = 1
    p = 4 + 9 * (4 + 8 * 40)                                  # a pocket: one free voxel whose neighbours are all occupied
    free[p] = 1
    for q in G.neighbours(p, dims):
        free[q] = 0
    cost = rs.randint(1, 9, size=n).astype(np.uint8)
    d = W.field(free, cost, dims, src)
    assert d[p] == W.NONE and W.locally_exact(d, free, cost, dims, src)
    reached = np.flatnonzero(d > 0)
    for v in reached[rs.randint(len(reached), size=12)]:
        for delta in (1, -1):
            bad = d.copy()
            bad[v] += delta
            assert not W.locally_exact(bad, free, cost, dims, src), (int(v), delta)
    bad = d.copy()
    bad[p] = 7                                                # an unreachable pocket given a value
    assert not W.locally_exact(bad, free, cost, dims, src)
    leaves = [int(v) for v in reached if all(d[q] <= d[v] for q in G.neighbours(int(v), dims))]
    bad = d.copy()
    bad[leaves[0]] = W.NONE                                   # a reachable voxel left out (nothing else depends on it)
    assert not W.locally_exact(bad, free, cost, dims, src)
    bad = d.copy()
    bad[np.flatnonzero(free == 0)[3]] = 4                     # a value on an occupied voxel
    assert not W.locally_exact(bad, free, cost, dims, src)
    bad = d.copy()
    bad[src] = 1
    assert not W.locally_exact(bad, free, cost, dims, src)
    other = W.field(free, cost, dims, int(reached[0]))        # a true field, of another source
    assert not W.locally_exact(other, free, cost, dims, src)


def test_clearance_costs_against_a_brute_force_count():
    rs = np.random.RandomState(4)
    for dims in ((7, 6, 5), (12, 3, 4), (5, 5, 1)):
        nx, ny, nz = dims
        n = nx * ny * nz
        free = (rs.uniform(size=n) >= 0.15).astype(np.uint8)
        d2 = CR.edt_brute(free, nx, ny, nz)
        for thr in ([1, 4, 9], [9, 1, 4], [], [0], [2, 2, 5], [1, 2, 3, 4, 5, 6, 7]):
            got = W.clearance_costs(free, d2, thr)
            for v in range(n):
                want = 0 if not free[v] else 1 + sum(1 for t in thr if d2[v] <= t)
                assert got[v] == want
            assert got.max() <= W.COST_MAX
    f3 = np.ones((1, 1, 9), np.uint8)
    f3[0, 0, 0] = 0
    d2 = CR.edt_brute(f3.reshape(-1), 9, 1, 1)
    assert W.clearance_costs(f3.reshape(-1), d2, [1, 4, 9]).tolist() == [0, 4, 3, 2, 1, 1, 1, 1, 1]
    empty = np.ones(24, np.uint8)
    d2 = CR.edt_brute(empty, 4, 3, 2)
    assert (d2 == W.D2_NONE).all() and (W.clearance_costs(empty, d2, [1, 4, 9]) == 1).all(), "no obstacle: cost 1 everywhere"


def ring_levels(free, cost, dims, src):
    """the kernel's scheme on boolean arrays: level L reads ring slot L mod (W + 1), settles it, touches the untouched free neighbours and
    schedules each for level L + its cost; the slot of level L + W is STORED (it held level L - 1), the others are ORed into"""
    nx, ny, nz = dims
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    c3 = np.asarray(cost).reshape(nz, ny, nx)
    Wm = int(c3[f3].max())
    R = Wm + 1
    ring = np.zeros((R, nz, ny, nx), bool)
    touched = np.zeros_like(f3)
    dist = np.full((nz, ny, nx), W.NONE, np.int32)
    z, y, x = int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx
    ring[0, z, y, x] = touched[z, y, x] = True
    level, idle = 0, 0
    while idle < R:
        fr = ring[level % R]
        dist[fr] = level
        nb = np.zeros_like(fr)
        nb[:, :, 1:] |= fr[:, :, :-1]
        nb[:, :, :-1] |= fr[:, :, 1:]
        nb[:, 1:, :] |= fr[:, :-1, :]
        nb[:, :-1, :] |= fr[:, 1:, :]
        nb[1:] |= fr[:-1]
        nb[:-1] |= fr[1:]
        T = nb & f3 & ~touched
        touched |= T
        idle = 0 if (fr.any() or T.any()) else idle + 1
        for k in range(1, Wm):
            ring[(level + k) % R] |= T & (c3 == k)
        ring[(level + Wm) % R] = T & (c3 == Wm)
        level += 1
    return dist.reshape(-1)


def test_the_level_scheme_is_dijkstra():
    rs = np.random.RandomState(21)
    for k in range(120):
        free, cost, dims = random_case(rs)
        cand = np.flatnonzero(free)
        s = int(cand[rs.randint(len(cand))])
        assert np.array_equal(ring_levels(free, cost, dims, s), W.field(free, cost, dims, s)), (k, dims)
