"""numpy restatement of the clearance-weighted shortest paths, written from the definitions in include/weldacs.h alone (section
"clearance-weighted exact shortest paths"): distances by a heap-based Dijkstra, the walk-back rule that defines THE path, the clearance
costs from the distance field of tests/clearance_ref.py, and a vectorised checker of the local conditions that only the exact field
satisfies (for fields too large for a Python heap).  Imports numpy and the other restatements only, so worker processes that use it
never open the GPU."""
import heapq

import numpy as np

from geodesic_ref import neighbours

NONE = -1        # WA_DIST_NONE
COST_MAX = 8     # WA_COST_MAX
D2_NONE = 0x7FFFFFFF


def field(free, cost, dims, src):
    """dist(src, v) for every voxel v as a flat int32 array in raster order: entering voxel v costs cost[v], the start is not paid for"""
    free = np.asarray(free).reshape(-1)
    cost = np.asarray(cost).reshape(-1)
    src = int(src)
    assert free[src], "an occupied source is an argument error"
    dist = np.full(free.size, NONE, np.int32)
    best = {src: 0}
    heap = [(0, src)]
    while heap:
        d, v = heapq.heappop(heap)
        if dist[v] >= 0:
            continue
        dist[v] = d
        for q in neighbours(v, dims):
            if free[q] and dist[q] < 0:
                nd = d + int(cost[q])
                if nd < best.get(q, 1 << 62):
                    best[q] = nd
                    heapq.heappush(heap, (nd, q))
    return dist


def fields(free, cost, dims, srcs):
    return np.stack([field(free, cost, dims, s) for s in srcs]) if len(srcs) else np.zeros((0, int(np.prod(dims))), np.int32)


def matrix(free, cost, dims, pts):
    pts = np.asarray(pts, np.int64)
    return np.stack([field(free, cost, dims, s)[pts] for s in pts]).astype(np.int32) if len(pts) else np.zeros((0, 0), np.int32)


def walk_back(dist, cost, dims, end):
    """the path start -> end given dist = field(free, cost, dims, start): None when end is not reachable"""
    D = int(dist[end])
    if D < 0:
        return None
    v = int(end)
    path = [v]
    while D > 0:
        want = D - int(cost[v])
        v = next(q for q in neighbours(v, dims) if dist[q] == want)   # (a voxel with a distance is free; want >= 0 is never NONE)
        path.append(v)
        D = want
    return np.array(path[::-1], np.int64)


def paths(free, cost, dims, starts, ends):
    """(dist int32[n], node counts int32[n] (0 when unreachable), [path or None])"""
    cache, dist, out = {}, [], []
    for s, e in zip(starts, ends):
        s, e = int(s), int(e)
        if s not in cache:
            cache[s] = field(free, cost, dims, s)
        dist.append(int(cache[s][e]))
        out.append(walk_back(cache[s], cost, dims, e))
    return np.array(dist, np.int32), np.array([0 if p is None else len(p) for p in out], np.int32), out


def path_cost(cost, path):
    """what a path pays: every node but the first"""
    return int(np.asarray(cost).reshape(-1).astype(np.int64)[np.asarray(path, np.int64)[1:]].sum())


def check_path(free, dims, path, start, end):
    """what a path must satisfy whichever rule picked it: start first, end last, every step a 6-neighbour step between free voxels"""
    free = np.asarray(free).reshape(-1)
    path = np.asarray(path, np.int64)
    assert len(path) >= 1 and path[0] == start and path[-1] == end
    assert (free[path] != 0).all()
    nx, ny, _ = dims
    a, b = path[:-1], path[1:]
    dx, dy, dz = b % nx - a % nx, (b // nx) % ny - (a // nx) % ny, b // (nx * ny) - a // (nx * ny)
    assert (abs(dx) + abs(dy) + abs(dz) == 1).all()


def clearance_costs(free, d2, thr2):
    """cost[v] = 0 on occupied voxels, else 1 + #{k : d2[v] <= thr2[k]}"""
    free = np.asarray(free).reshape(-1)
    d2 = np.asarray(d2, np.int64).reshape(-1)
    c = np.ones(free.size, np.int64)
    for t in thr2:
        c += d2 <= int(t)
    return np.where(free != 0, c, 0).astype(np.uint8)


def locally_exact(dist, free, cost, dims, src, slab=32):
    """True iff dist is THE field of src: dist[src] = 0; every other free voxel with d >= 0 has d = cost + the smallest d >= 0 among
    its neighbours, and has such a neighbour; a free voxel with d < 0 has no neighbour with d >= 0; occupied voxels hold -1.
    Costs are positive, so following the smallest neighbour strictly decreases d and must end at the only voxel exempt from the rule,
    the source: d is the cost of a real path, d >= the distance; and d <= cost + d of EVERY neighbour gives d <= the distance by
    induction along a shortest path.  The third condition makes the reached set the source's whole component."""
    nx, ny, nz = dims
    dist = np.asarray(dist).reshape(-1)
    free = np.asarray(free).reshape(-1)
    cost = np.asarray(cost).reshape(-1)
    if dist[src] != 0 or (dist[free == 0] != NONE).any():
        return False
    d3 = dist.reshape(nz, ny, nx)
    f3 = free.reshape(nz, ny, nx) != 0
    c3 = cost.reshape(nz, ny, nx)
    BIG = np.int64(1) << 40
    sz, sy, sx = int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx
    for z0 in range(0, nz, slab):
        z1 = min(nz, z0 + slab)
        a, b = max(z0 - 1, 0), min(z1 + 1, nz)
        big = np.where(d3[a:b] >= 0, d3[a:b].astype(np.int64), BIG)
        lo = np.full_like(big, BIG)
        np.minimum(lo[:, :, 1:], big[:, :, :-1], out=lo[:, :, 1:])
        np.minimum(lo[:, :, :-1], big[:, :, 1:], out=lo[:, :, :-1])
        np.minimum(lo[:, 1:, :], big[:, :-1, :], out=lo[:, 1:, :])
        np.minimum(lo[:, :-1, :], big[:, 1:, :], out=lo[:, :-1, :])
        np.minimum(lo[1:], big[:-1], out=lo[1:])
        np.minimum(lo[:-1], big[1:], out=lo[:-1])
        lo, d, f, c = lo[z0 - a:z0 - a + (z1 - z0)], d3[z0:z1], f3[z0:z1], c3[z0:z1]
        rule = f & (d >= 0)
        if z0 <= sz < z1:
            rule = rule.copy()
            rule[sz - z0, sy, sx] = False
        if not np.array_equal(lo[rule] + c[rule], d[rule].astype(np.int64)):     # (no neighbour: BIG + cost != d)
            return False
        if (lo[f & (d < 0)] != BIG).any():
            return False
    return True


def scipy_fields(free, cost, dims, srcs):
    """the same distances by scipy.sparse.csgraph.dijkstra on the directed graph with edge u -> v weighted cost[v]"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    nx, ny, nz = dims
    n = nx * ny * nz
    free = np.asarray(free).reshape(-1) != 0
    cost = np.asarray(cost).reshape(-1)
    ids = np.arange(n, dtype=np.int64).reshape(nz, ny, nx)
    us, vs = [], []
    for a, b in ((ids[:, :, :-1], ids[:, :, 1:]), (ids[:, :-1, :], ids[:, 1:, :]), (ids[:-1], ids[1:])):
        a, b = a.reshape(-1), b.reshape(-1)
        ok = free[a] & free[b]
        us += [a[ok], b[ok]]
        vs += [b[ok], a[ok]]
    u, v = np.concatenate(us), np.concatenate(vs)
    g = csr_matrix((cost[v].astype(np.float64), (u, v)), shape=(n, n))
    d = dijkstra(g, directed=True, indices=np.asarray(srcs, np.int64))
    out = np.where(np.isfinite(d), d, NONE).astype(np.int32)
    return out.reshape(len(srcs), n)


def hand_cases():
    """(name, free, cost, dims, source, {voxel: dist}, {end: path}) -- answers worked out by hand from the definition"""
    cases = []
    # a corridor 7 x 1 x 1 whose voxel 3 costs 8: no way round, it is paid for
    cases.append(("corridor_pays_the_toll", np.ones(7, np.uint8), np.array([1, 1, 1, 8, 1, 1, 1], np.uint8), (7, 1, 1), 0,
                  {0: 0, 1: 1, 2: 2, 3: 10, 4: 11, 5: 12, 6: 13}, {6: [0, 1, 2, 3, 4, 5, 6], 0: [0]}))
    # 5 x 2 x 1, all free; row 0 (ids 0..4) costs 1 1 8 1 1, row 1 (ids 5..9) all 1: from 0 to 4 the detour through row 1 costs 6 in
    # 6 steps, the straight line 11 in 4; voxel 2 itself is entered from 1: 1 + 8 = 9
    cost = np.array([1, 1, 8, 1, 1,
                     1, 1, 1, 1, 1], np.uint8)
    cases.append(("detour_round_the_expensive_cell", np.ones(10, np.uint8), cost, (5, 2, 1), 0,
                  {0: 0, 1: 1, 5: 1, 6: 2, 7: 3, 8: 4, 9: 5, 3: 5, 4: 6, 2: 9},
                  {4: [0, 5, 6, 7, 8, 3, 4], 2: [0, 1, 2], 9: [0, 5, 6, 7, 8, 9]}))
    # the same pair from the other end with cost[0] = 3: dist(4, 0) = dist(0, 4) + cost[0] - cost[4] = 6 + 2.  Walking back from 0 with
    # D = 8, want 5: +x neighbour 1 holds 5 (4 -> 9 -> 8 -> 7 -> 6 -> 1) and comes before +y neighbour 5, which holds 5 as well
    cost2 = cost.copy()
    cost2[0] = 3
    cases.append(("asymmetry", np.ones(10, np.uint8), cost2, (5, 2, 1), 4,
                  {4: 0, 0: 8, 3: 1, 9: 1, 5: 5, 1: 5, 2: 9}, {0: [4, 9, 8, 7, 6, 1, 0]}))
    return cases


def tie_case():
    """3 x 3 x 1, all free, costs 1 except the centre (4) = 2; from voxel 0 to voxel 8 every monotone path round the centre costs 4 and
    the ones through it cost 5.  Walking back from 8 = (2, 2): D = 4, want 3: -x neighbour 7 = (1, 2) has 3: taken (before 5 = (2, 1),
    which has 3 as well).  From 7, want 2: -x neighbour 6 = (0, 2) has 2: taken; the centre holds 3.  Then 3, then 0."""
    cost = np.ones(9, np.uint8)
    cost[4] = 2
    return np.ones(9, np.uint8), cost, (3, 3, 1), 0, 8, [0, 3, 6, 7, 8]
