"""numpy restatement of the penalised 26-neighbour chamfer fields, written from the definitions in include/weldacs.h alone (section "exact
shortest paths with diagonal moves and clearance penalties"): the move u -> v costs step[class - 1] + pen[v].  Distances by a heap-based
Dijkstra, the walk-back rule that defines THE path, the cost of any path under the metric, the two-stage ring of settled sets on boolean
arrays (the algorithm the device runs, held against the Dijkstra by tests/test_chamfer_weighted_rules.py) and hand cases.  The graph, the
box rule and the offset order come from tests/chamfer_ref.py.  Imports numpy and the other restatements only, so worker processes that
use it never open the GPU."""
import heapq

import numpy as np

import chamfer_ref as C

NONE = -1        # WA_DIST_NONE
PEN_MAX = 31     # WA_PEN_MAX


def field(free, step, pen, dims, src, moves=None):
    """dist(src, v) for every voxel v as a flat int32 array in raster order, by Dijkstra with a heap; the start is not paid for"""
    free = np.asarray(free).reshape(-1)
    pen = np.asarray(pen).reshape(-1)
    src = int(src)
    assert free[src], "an occupied source is an argument error"
    moves = moves or C._flat_moves(free, dims)
    nb = [[] for _ in range(free.size)]
    for (d, ok), cls in zip(moves, C.CLASS):
        for v in np.flatnonzero(ok).tolist():
            nb[v].append((v + d, int(step[cls - 1]) + int(pen[v + d])))
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


def fields(free, step, pen, dims, srcs):
    if not len(srcs):
        return np.zeros((0, int(np.prod(dims))), np.int32)
    moves = C._flat_moves(free, dims)
    return np.stack([field(free, step, pen, dims, s, moves) for s in srcs])


def matrix(free, step, pen, dims, pts):
    pts = np.asarray(pts, np.int64)
    return fields(free, step, pen, dims, pts)[:, pts].astype(np.int32) if len(pts) else np.zeros((0, 0), np.int32)


def ring_field(free, step, pen, dims, src):
    """the same field by the two-stage ring: R = M + P + 1 sets, slot L mod R = the voxels whose distance is L.  Level L = 1, 2, ...:
    cand = chamfer_ref.ring_field's pull from slots L - step; A = cand & ~arrived; the voxels of A with penalty P REPLACE slot L + P (it
    held the set of L - M - 1), those with penalty q < P are ORed into slot L + q, and all get L + q at once.  Finished when M + P
    levels in a row had no arrival."""
    nx, ny, nz = dims
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    p3 = np.where(f3, np.asarray(pen).reshape(nz, ny, nx), 0).astype(np.int64)
    ok = C.allowed_moves(free, dims)
    M, P = int(max(step)), int(p3.max())
    R = M + P + 1
    ring = [np.zeros((nz, ny, nx), bool) for _ in range(R)]
    z, y, x = int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx
    ring[0][z, y, x] = True
    arrived = ring[0].copy()
    dist = np.full((nz, ny, nx), NONE, np.int32)
    dist[z, y, x] = 0
    L, last = 1, 0
    while last >= L - (M + P):
        cand = np.zeros((nz, ny, nx), bool)
        for o, a, cls in zip(C.OFFSETS, ok, C.CLASS):
            c = int(step[cls - 1])
            if L >= c:
                cand |= C.shifted(ring[(L - c) % R], o) & a
        A = cand & f3 & ~arrived
        ring[(L + P) % R] = A & (p3 == P)
        if A.any():
            arrived |= A
            last = L
            for q in range(P):
                m = A & (p3 == q)
                if m.any():
                    ring[(L + q) % R] |= m
            dist[A] = L + p3[A]
        L += 1
    return dist.reshape(-1)


def walk_back(dist, free, step, pen, dims, end, moves=None):
    """the path start -> end given dist = field(free, step, pen, dims, start): None when end is not reachable"""
    D = int(dist[end])
    if D < 0:
        return None
    pen = np.asarray(pen).reshape(-1)
    moves = moves or C._flat_moves(free, dims)
    v = int(end)
    path = [v]
    while D > 0:
        for (d, ok), cls in zip(moves, C.CLASS):
            want = D - int(pen[v]) - int(step[cls - 1])
            if want >= 0 and ok[v] and dist[v + d] == want:
                v, D = v + d, want
                break
        else:
            raise AssertionError("a voxel with a distance has a predecessor")
        path.append(v)
    return np.array(path[::-1], np.int64)


def paths(free, step, pen, dims, starts, ends):
    """(dist int32[n], node counts int32[n] (0 when unreachable), [path or None])"""
    moves = C._flat_moves(free, dims)
    cache, dist, out = {}, [], []
    for s, e in zip(starts, ends):
        s, e = int(s), int(e)
        if s not in cache:
            cache[s] = field(free, step, pen, dims, s, moves)
        dist.append(int(cache[s][e]))
        out.append(walk_back(cache[s], free, step, pen, dims, e, moves))
    return np.array(dist, np.int32), np.array([0 if p is None else len(p) for p in out], np.int32), out


def path_cost(step, pen, dims, path):
    """what any 26-neighbour path pays under the metric: the step of every move and the penalty of every node but the first"""
    path = np.asarray(path, np.int64)
    return C.path_cost(step, dims, path) + int(np.asarray(pen).reshape(-1).astype(np.int64)[path[1:]].sum())


def strip(step):
    """the 65 x 3 x 1 strip, all free, row y = 1 with penalty 31 between two rows of penalty 0, from voxel 0: the front runs along row 0
    and the voxels of row 1 settle 31 levels behind it.  With f, e = step[0], step[1] and e <= 2 f: row 0 holds f x; (x, 1) is reached
    cheapest by the edge move from (x - 1, 0), f (x - 1) + e + 31 (the face move from (0, 0) for x = 0: f + 31); (x, 2) for x >= 2 by
    the edge move from (x - 1, 1).  Returns (free, pen, dims, {voxel: dist})."""
    f, e = int(step[0]), int(step[1])
    dims = (65, 3, 1)
    pen = np.zeros(195, np.uint8)
    pen[65:130] = 31
    row1 = lambda x: f + 31 if x == 0 else f * (x - 1) + e + 31
    row2 = lambda x: min(row1(0) + f, row1(1) + e) if x == 0 else min(row1(x - 1) + e, row1(x) + f)
    want = {0: 0, 3: 3 * f, 64: 64 * f, 65: row1(0), 70: row1(5), 129: row1(64), 130: row2(0), 131: row2(1), 140: row2(10), 194: row2(64)}
    return np.ones(195, np.uint8), pen, dims, want


def hand_cases():
    """(name, free, step, pen, dims, source, {voxel: dist}, {end: path}) -- answers worked out on paper from the definition"""
    cases = []
    for step in ((3, 4, 5), (16, 16, 16), (1, 1, 1)):
        free, pen, dims, want = strip(step)
        # walking back from (5, 1) = 70: no face neighbour holds D - 31 - f; the first edge offset (-1, -1, 0) leads to (4, 0), which does;
        # row 0 is then walked by -x moves.  With {16, 16, 16} and {1, 1, 1} the same: (5, 0) holds D - 31 exactly, not D - 31 - f
        cases.append(("strip_%d_%d_%d" % step, free, step, pen, dims, 0, want, {70: [0, 1, 2, 3, 4, 70], 3: [0, 1, 2, 3]}))
    # chamfer_ref's {16, 1, 7} box (2 x 2 x 2, all free, id = x + 2 y + 4 z) from 0 with pen[1] = 5, pen[3] = 2, pen[7] = 1.  Edge moves
    # cost 1: 5 and 6 hold 1, 3 holds 1 + 2.  The odd voxels need a corner move (7) or a face move (16): 2 = corner from 5 = 8; 7 = corner
    # from 0 = 7 + 1; 4 = edge from 2 (or 7) = 9; 1 = corner from 6 = 1 + 7 + 5 = 13 (the edges from 2 and 7 give 8 + 1 + 5).
    # Walking back from 1, D = 13: D - 5 = 8; no face; no voxel holds 7; the only corner neighbour 6 holds 1 = 8 - 7.  From 6, D = 1: the
    # edge offset (0, -1, -1) leads to 0.  From 4, D = 9: edges want 8: (1, 0, -1) -> 1 holds 13, (0, 1, -1) -> 2 holds 8: taken; from 2
    # the corner neighbour 5 holds 1 = 8 - 7; from 5 the edge (-1, 0, -1) leads to 0.
    pen = np.array([0, 5, 0, 2, 0, 0, 0, 1], np.uint8)
    cases.append(("penalties_in_the_16_1_7_box", np.ones(8, np.uint8), (16, 1, 7), pen, (2, 2, 2), 0,
                  {0: 0, 5: 1, 6: 1, 3: 3, 2: 8, 7: 8, 4: 9, 1: 13}, {1: [0, 6, 1], 4: [0, 5, 2, 4], 3: [0, 3]}))
    # 3 x 2 x 1, all free, {3, 4, 5}, pen 9 on voxel 1 = (1, 0): from 0 to 2 the straight line costs 3 + 9 + 3, the way over row 1 by two
    # edge moves 4 + 4: voxel 1 itself is entered from 0 for 12.  Walking back from 2, D = 8: faces want 5: 1 holds 12, 5 = (2, 1) holds
    # 7 (edge 0 -> 4, face 4 -> 5); edges want 4: (-1, 1, 0) -> 4 holds 4.
    pen = np.array([0, 9, 0, 0, 0, 0], np.uint8)
    cases.append(("round_the_penalised_voxel", np.ones(6, np.uint8), (3, 4, 5), pen, (3, 2, 1), 0,
                  {0: 0, 1: 12, 3: 3, 4: 4, 5: 7, 2: 8}, {2: [0, 4, 2], 1: [0, 1]}))
    return cases
