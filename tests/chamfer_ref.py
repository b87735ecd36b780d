"""numpy restatement of the 26-neighbour chamfer fields, written from the definitions in include/weldacs.h alone (section "exact shortest
paths with diagonal moves"): the box rule, distances by a heap-based Dijkstra, the walk-back rule that defines THE path, the pull-form
ring of settled sets on boolean arrays (the algorithm the device runs, held against the Dijkstra by tests/test_chamfer_rules.py), and a
vectorised checker of the local conditions that only the exact field satisfies.  Imports numpy only, so worker processes that use it
never open the GPU."""
import heapq

import numpy as np

NONE = -1        # WA_DIST_NONE
STEP_MAX = 16    # WA_STEP_MAX

# the fixed order of the walk-back: the six face offsets -x, +x, -y, +y, -z, +z, then the edge offsets, then the corner offsets, the last
# two sorted by (dz, dy, dx) ascending.  Entries are (dx, dy, dz).
_ALL = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
_CLS = lambda o: sum(1 for c in o if c)
OFFSETS = ([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
           + [o for o in _ALL if _CLS(o) == 2] + [o for o in _ALL if _CLS(o) == 3])
CLASS = [_CLS(o) for o in OFFSETS]
assert len(OFFSETS) == 26 and CLASS == [1] * 6 + [2] * 12 + [3] * 8


def shifted(a3, o):
    """b[z, y, x] = a3[z + dz, y + dy, x + dx], False where that lies outside the grid"""
    dx, dy, dz = o
    nz, ny, nx = a3.shape
    b = np.zeros_like(a3)
    zs, zd = slice(max(dz, 0), nz + min(dz, 0)), slice(max(-dz, 0), nz + min(-dz, 0))
    ys, yd = slice(max(dy, 0), ny + min(dy, 0)), slice(max(-dy, 0), ny + min(-dy, 0))
    xs, xd = slice(max(dx, 0), nx + min(dx, 0)), slice(max(-dx, 0), nx + min(-dx, 0))
    b[zd, yd, xd] = a3[zs, ys, xs]
    return b


def allowed_moves(free, dims):
    """[26] boolean arrays (nz, ny, nx) in the order of OFFSETS: [k][p] = the move p -> p + OFFSETS[k] exists, that is all 2^class voxels
    of the box the two span are inside the grid and free"""
    nx, ny, nz = dims
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    out = []
    for dx, dy, dz in OFFSETS:
        ok = f3.copy()
        for ax in sorted({0, dx}):
            for ay in sorted({0, dy}):
                for az in sorted({0, dz}):
                    ok &= shifted(f3, (ax, ay, az))
        out.append(ok)
    return out


def move_exists(free, dims, u, v):
    """the definition, voxel by voxel (what allowed_moves vectorises)"""
    nx, ny, nz = dims
    free = np.asarray(free).reshape(-1)
    cu = (u % nx, (u // nx) % ny, u // (nx * ny))
    cv = (v % nx, (v // nx) % ny, v // (nx * ny))
    if u == v or max(abs(a - b) for a, b in zip(cu, cv)) > 1:
        return False
    return all(free[x + nx * (y + ny * z)] for x in {cu[0], cv[0]} for y in {cu[1], cv[1]} for z in {cu[2], cv[2]})


def forbidden_moves(free, dims):
    """how many ordered pairs of free 26-neighbours have no move between them: what the box rule forbids"""
    nx, ny, nz = dims
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    return int(sum((f3 & shifted(f3, o) & ~ok).sum() for o, ok in zip(OFFSETS, allowed_moves(free, dims))))


def _flat_moves(free, dims):
    nx, ny, _ = dims
    return [(dx + nx * (dy + ny * dz), ok.reshape(-1)) for (dx, dy, dz), ok in zip(OFFSETS, allowed_moves(free, dims))]


def field(free, step, dims, src, moves=None):
    """dist(src, v) for every voxel v as a flat int32 array in raster order, by Dijkstra with a heap"""
    free = np.asarray(free).reshape(-1)
    src = int(src)
    assert free[src], "an occupied source is an argument error"
    moves = moves or _flat_moves(free, dims)
    nb = [[] for _ in range(free.size)]
    for (d, ok), cls in zip(moves, CLASS):
        for v in np.flatnonzero(ok).tolist():
            nb[v].append((v + d, int(step[cls - 1])))
    dist = np.full(free.size, NONE, np.int32)
    best = {src: 0}
    heap = [(0, src)]
    while heap:
        d, v = heapq.heappop(heap)
        if dist[v] >= 0:
            continue
        dist[v] = d
        for q, c in nb[v]:
            if dist[q] < 0 and d + c < best.get(q, 1 << 62):
                best[q] = d + c
                heapq.heappush(heap, (d + c, q))
    return dist


def fields(free, step, dims, srcs):
    if not len(srcs):
        return np.zeros((0, int(np.prod(dims))), np.int32)
    moves = _flat_moves(free, dims)
    return np.stack([field(free, step, dims, s, moves) for s in srcs])


def matrix(free, step, dims, pts):
    pts = np.asarray(pts, np.int64)
    return fields(free, step, dims, pts)[:, pts].astype(np.int32) if len(pts) else np.zeros((0, 0), np.int32)


def ring_field(free, step, dims, src):
    """the same field by the pull form over a ring of settled sets: S_L = (union over the offsets o of [S_{L - step[class(o)]} seen at
    p + o] & [the move exists]) & ~done, for L = 1, 2, ...; finished when max(step) levels in a row have settled nothing"""
    nx, ny, nz = dims
    ok = allowed_moves(free, dims)
    M = int(max(step))
    R = M + 1
    ring = [np.zeros((nz, ny, nx), bool) for _ in range(R)]
    z, y, x = int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx
    ring[0][z, y, x] = True
    done = ring[0].copy()
    dist = np.full((nz, ny, nx), NONE, np.int32)
    dist[z, y, x] = 0
    L, last = 1, 0
    while last >= L - M:
        cand = np.zeros((nz, ny, nx), bool)
        for o, a, cls in zip(OFFSETS, ok, CLASS):
            c = int(step[cls - 1])
            if L >= c:
                cand |= shifted(ring[(L - c) % R], o) & a
        S = cand & ~done
        ring[L % R] = S
        if S.any():
            done |= S
            dist[S] = L
            last = L
        L += 1
    return dist.reshape(-1)


def walk_back(dist, free, step, dims, end, moves=None):
    """the path start -> end given dist = field(free, step, dims, start): None when end is not reachable"""
    D = int(dist[end])
    if D < 0:
        return None
    moves = moves or _flat_moves(free, dims)
    v = int(end)
    path = [v]
    while D > 0:
        for (d, ok), cls in zip(moves, CLASS):
            want = D - int(step[cls - 1])
            if want >= 0 and ok[v] and dist[v + d] == want:     # (the rule is symmetric: v -> v + d exists iff v + d -> v does)
                v, D = v + d, want
                break
        else:
            raise AssertionError("a voxel with a distance has a predecessor")
        path.append(v)
    return np.array(path[::-1], np.int64)


def paths(free, step, dims, starts, ends):
    """(dist int32[n], node counts int32[n] (0 when unreachable), [path or None])"""
    moves = _flat_moves(free, dims)
    cache, dist, out = {}, [], []
    for s, e in zip(starts, ends):
        s, e = int(s), int(e)
        if s not in cache:
            cache[s] = field(free, step, dims, s, moves)
        dist.append(int(cache[s][e]))
        out.append(walk_back(cache[s], free, step, dims, e, moves))
    return np.array(dist, np.int32), np.array([0 if p is None else len(p) for p in out], np.int32), out


def move_classes(dims, path):
    """the class (1, 2, 3) of every move of a path; asserts that each is a 26-neighbour move"""
    nx, ny, _ = dims
    path = np.asarray(path, np.int64)
    a, b = path[:-1], path[1:]
    dx, dy, dz = b % nx - a % nx, (b // nx) % ny - (a // nx) % ny, b // (nx * ny) - a // (nx * ny)
    assert (np.maximum(np.maximum(abs(dx), abs(dy)), abs(dz)) == 1).all() if len(a) else True
    return (dx != 0).astype(np.int64) + (dy != 0) + (dz != 0)


def moves_by_class(dims, path):
    return np.bincount(move_classes(dims, path), minlength=4)[1:4]


def path_cost(step, dims, path):
    return int((np.asarray(step, np.int64)[move_classes(dims, path) - 1]).sum())


def check_path(free, dims, path, start, end):
    """what a path must satisfy whichever rule picked it: start first, end last, every step a 26-neighbour move whose box is free"""
    free = np.asarray(free).reshape(-1)
    path = np.asarray(path, np.int64)
    assert len(path) >= 1 and path[0] == start and path[-1] == end
    assert (free[path] != 0).all()
    move_classes(dims, path)
    for a, b in zip(path[:-1].tolist(), path[1:].tolist()):
        assert move_exists(free, dims, a, b), (a, b)


def locally_exact(dist, free, step, dims, src):
    """True iff dist is THE field of src: dist[src] = 0; every other free voxel with d >= 0 has d = the smallest (d of q) + step over its
    existing moves to voxels q with a distance, and has such a move; a free voxel with d < 0 has no move to a voxel with d >= 0; occupied
    voxels hold -1.  Steps are positive, so following the minimising move strictly decreases d and must end at the only voxel exempt from
    the rule, the source: d is the cost of a real path, d >= the distance; and d <= step + d of EVERY neighbour gives d <= the distance
    by induction along a shortest path.  The third condition makes the reached set the source's whole component."""
    nx, ny, nz = dims
    dist = np.asarray(dist).reshape(-1)
    free = np.asarray(free).reshape(-1)
    if dist[src] != 0 or (dist[free == 0] != NONE).any():
        return False
    d3 = dist.reshape(nz, ny, nx)
    f3 = free.reshape(nz, ny, nx) != 0
    BIG = np.int64(1) << 40
    big = np.where(d3 >= 0, d3.astype(np.int64), BIG)
    lo = np.full((nz, ny, nx), BIG, np.int64)
    pad = np.full((nz + 2, ny + 2, nx + 2), BIG, np.int64)
    pad[1:-1, 1:-1, 1:-1] = big
    for (dx, dy, dz), ok, cls in zip(OFFSETS, allowed_moves(free, dims), CLASS):
        nb = pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        np.minimum(lo, np.where(ok, nb + int(step[cls - 1]), BIG), out=lo)
    lo = np.minimum(lo, BIG)
    rule = f3 & (d3 >= 0)
    rule[int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx] = False
    if not np.array_equal(lo[rule], d3[rule].astype(np.int64)):
        return False
    return not (lo[f3 & (d3 < 0)] < BIG).any()


def chebyshev(dims, src):
    nx, ny, nz = dims
    v = np.arange(nx * ny * nz)
    d = np.stack([abs(v % nx - src % nx), abs((v // nx) % ny - (src // nx) % ny), abs(v // (nx * ny) - src // (nx * ny))])
    return d


def closed_form(step, dims, src):
    """dist on a grid without obstacles for the two triples that have one: {1, 1, 1} (Chebyshev) and {3, 4, 5}"""
    a = np.sort(chebyshev(dims, src), axis=0)[::-1]
    if tuple(step) == (1, 1, 1):
        return a[0].astype(np.int32)
    assert tuple(step) == (3, 4, 5)
    return (3 * (a[0] - a[1]) + 4 * (a[1] - a[2]) + 5 * a[2]).astype(np.int32)


def hand_cases():
    """(name, free, step, dims, source, {voxel: dist}, {end: path}) -- answers worked out on paper from the definition"""
    cases = []
    # 2 x 2 x 1, ids 0 = (0,0), 1 = (1,0), 2 = (0,1), 3 = (1,1) occupied.  The diagonal 1 <-> 2 spans the box {0, 1, 2, 3}: forbidden, so
    # from 1 voxel 2 is reached through 0 for 3 + 3, not for 4
    cases.append(("diagonal_forbidden_by_the_occupied_corner", np.array([1, 1, 1, 0], np.uint8), (3, 4, 5), (2, 2, 1), 1,
                  {1: 0, 0: 3, 2: 6, 3: NONE}, {2: [1, 0, 2], 1: [1]}))
    # the same box all free: the diagonal exists and costs 4
    cases.append(("diagonal_allowed_in_the_free_box", np.ones(4, np.uint8), (3, 4, 5), (2, 2, 1), 1,
                  {1: 0, 0: 3, 3: 3, 2: 4}, {2: [1, 2]}))
    # a tie the face-first order decides: 2 x 2 x 1 all free with step {1, 2, 3}: 0 -> 3 costs 2 by the diagonal and 2 by two face
    # moves.  Walking back from 3 = (1,1), D = 2: -x neighbour 2 = (0,1) holds 1 = 2 - 1 and is asked first: the path is 0, 2, 3
    cases.append(("tie_goes_to_the_face_move", np.ones(4, np.uint8), (1, 2, 3), (2, 2, 1), 0,
                  {0: 0, 1: 1, 2: 1, 3: 2}, {3: [0, 2, 3]}))
    # step {16, 1, 7} in a free 2 x 2 x 2 box (id = x + 2 y + 4 z) from 0: edge moves (cost 1) keep the parity of x + y + z, so the face
    # neighbours 1, 2, 4 and the corner 7 need one odd move: 7 = the corner move (7), 1 = corner + edge = 8, not the face move's 16.
    # Voxel 1 is touched by the face move from the source at once and settles only at level 8, from voxels that settled at 7 and at 1.
    # Walking back from 1 = (1,0,0), D = 8: no face (8 - 16 < 0); edges want 7: (0,1,-1) -> 2 holds 8, (1,0,-1) -> 4 holds 8,
    # (1,1,0) -> 7 holds 7: taken.  From 7, D = 7: edges want 6 (3, 5, 6 hold 1), corners want 0: (-1,-1,-1) -> 0.
    cases.append(("settles_later_from_a_cheap_move", np.ones(8, np.uint8), (16, 1, 7), (2, 2, 2), 0,
                  {0: 0, 3: 1, 5: 1, 6: 1, 7: 7, 1: 8, 2: 8, 4: 8}, {1: [0, 7, 1], 7: [0, 7], 3: [0, 3]}))
    # 3 x 3 x 1 with the centre occupied, {3, 4, 5}: every diagonal of the ring touches the centre's box, so the ring is walked by face
    # moves only: from 0 = (0,0) to 8 = (2,2) it is 4 face moves = 12
    f = np.ones(9, np.uint8)
    f[4] = 0
    cases.append(("ring_round_an_occupied_centre", f, (3, 4, 5), (3, 3, 1), 0,
                  {0: 0, 1: 3, 2: 6, 5: 9, 8: 12, 3: 3, 6: 6, 7: 9, 4: NONE}, {8: [0, 3, 6, 7, 8]}))
    return cases
