"""numpy restatement of the turn-cost pose paths of include/weldacs.h (wa_grid_pose_weighted_fields, _matrix, _paths; rules 30 - 36 of
the torch section), written from the header's definition and independent of the kernels: the states, seeds and adjacency are
pose_ref.Scene's, a step (v, k) -> (v', k') costs hop + turn_costs[class(k, k')] + pen[v'].  The search is level-synchronous with the
level the distance (every step costs at least 1), as pose_ref.Scene.levels is for hops; heap_dist() is the independent check, a binary
heap over explicit states."""
import heapq

import numpy as np

import geodesic_ref as GR
import pose_ref as PR
import torch_ref as TR

NONE = -1            # WA_DIST_NONE
MAX_BANDS, COST_MAX = 4, 15


class Costs:
    """rule 30: hop 1 .. 8, B = len(bands) <= 4 strictly ascending, turn_costs [B + 1] non-decreasing from 0, pen uint8 [n] or None"""

    def __init__(self, hop, bands=(), turn_costs=(0,), pen=None):
        self.hop, self.bands, self.turn_costs = int(hop), [int(b) for b in bands], [int(c) for c in turn_costs]
        self.pen = None if pen is None else np.asarray(pen, np.uint8).ravel()
        assert 1 <= self.hop <= 8 and len(self.bands) <= MAX_BANDS and len(self.turn_costs) == len(self.bands) + 1
        assert all(0 <= b <= PR.MAX_TURN for b in self.bands) and all(a < b for a, b in zip(self.bands, self.bands[1:]))
        assert self.turn_costs[0] == 0 and max(self.turn_costs) <= COST_MAX
        assert all(a <= b for a, b in zip(self.turn_costs, self.turn_costs[1:]))

    def scaled(self, f):
        return Costs(self.hop * f, self.bands, [c * f for c in self.turn_costs], None if self.pen is None else self.pen * f)


def turn_class(dirs, bands):
    """class(k, k') as int64 [K, K] (rule 31): the number of bands U exceeds"""
    q = TR.quantise_all(dirs)
    U = TR.turn(q[:, None, :], q[None, :, :])
    return (U[:, :, None] > np.asarray(bands, np.int64).reshape(1, 1, -1)).sum(2)


def bands_for(dirs, max_turn, B):
    """B integer thresholds at quantiles of U over the adjacent pairs k != k', such that every class 1 .. B holds an adjacent pair"""
    q = TR.quantise_all(dirs)
    U = TR.turn(q[:, None, :], q[None, :, :])
    adj = PR.adjacency(dirs, max_turn) & ~np.eye(len(q), dtype=bool)
    vals = np.unique(U[adj])
    assert len(vals) > B, "too few distinct turns among the adjacent pairs for %d bands" % B
    bands = [int(vals[(b * len(vals)) // (B + 1)]) for b in range(B)]
    cls = turn_class(dirs, bands)
    assert all(a < b for a, b in zip(bands, bands[1:]))
    assert all((adj & (cls == c)).any() for c in range(1, B + 1)), "a class without an adjacent pair"
    return bands


def bands_upto(dirs, max_turn, B):
    """bands_for with the most bands up to B that the directions can fill (a small K has few distinct turns)"""
    for b in range(B, 0, -1):
        try:
            return bands_for(dirs, max_turn, b)
        except AssertionError:
            pass
    return []


class Scene:
    """what every search of one (grid, dirs, tool, max_turn, costs) shares.  base: a pose_ref.Scene of the same grid, dirs and tool
    (its open(v, k) is reused)"""

    def __init__(self, grid, dirs, tool, max_turn, costs, base=None):
        self.base = (PR.Scene(grid, dirs, tool, max_turn) if base is None else
                     base if base.max_turn == max_turn else base.with_turn(max_turn))
        self.costs = costs
        self.dims, self.n, self.K = self.base.dims, self.base.n, self.base.K
        self.opened, self.adj, self.free = self.base.opened, self.base.adj, self.base.free
        self.pen = np.zeros(self.n, np.int64) if costs.pen is None else np.where(self.free, costs.pen.astype(np.int64), 0)
        assert len(self.pen) == self.n and self.pen.max() <= COST_MAX
        self.cls = turn_class(self.base.dirs, costs.bands)
        self.step = costs.hop + np.asarray(costs.turn_costs, np.int64)[self.cls]      # [K, K], meaningful where adj
        self.P = int(self.pen[self.free].max()) if self.free.any() else 0
        self.R = costs.hop + max(costs.turn_costs) + self.P + 1
        self.weights = sorted({int(w) for w in self.step[self.adj]})
        self.max_level = 0
        self._fields = {}

    # Sets of states travel as the header's masks do: bit (k & 63) of word [k >> 6, v] (rule 11's packing), so that what touches
    # every voxel at every level is a handful of 64-bit operations; single states are unpacked only around the front.
    def pack(self, bits):
        """bool [r, K] -> uint64 [W, r]"""
        out = np.zeros(((self.K + 63) // 64, len(bits)), np.uint64)
        for w in range(len(out)):
            part = bits[:, 64 * w:64 * w + 64].astype(np.uint64)
            out[w] = (part << np.arange(part.shape[1], dtype=np.uint64)).sum(1, dtype=np.uint64)      # distinct bits: the sum is the OR
        return out

    def unpack(self, words):
        """uint64 [W, r] -> bool [r, K]"""
        k = np.arange(self.K)
        return ((words[k >> 6].T >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)

    def neighbour_or(self, words):
        """uint64 [W, n] -> the OR over the six neighbours of every voxel"""
        nx, ny, nz = self.dims
        f = words.reshape(-1, nz, ny, nx)
        m = np.zeros_like(f)
        m[:, :, :, 1:] |= f[:, :, :, :-1]
        m[:, :, :, :-1] |= f[:, :, :, 1:]
        m[:, :, 1:] |= f[:, :, :-1]
        m[:, :, :-1] |= f[:, :, 1:]
        m[:, 1:] |= f[:, :-1]
        m[:, :-1] |= f[:, 1:]
        return m.reshape(len(words), -1)

    def levels(self, src, pin=-1):
        """(state int32 [K, n]: dist(s; v, k) at [k, v], cost int32 [n]) of the source (src, pin); kept, and never modified.  The sets
        of the last R - 1 levels are kept as what they offer the neighbours of their voxels."""
        key = (int(src), int(pin))
        if key in self._fields:
            return self._fields[key]
        seed = self.base.seed(int(src), int(pin))
        state = np.full((self.n, self.K), NONE, np.int32)
        state[seed] = 0
        opened, seen = self.pack(self.opened), self.pack(seed)
        rows_of = [(w, self.pack(self.adj & (self.step == w))) for w in self.weights]      # [W, K]: who reaches k with a step of w
        pens = [(int(p), self.pen == p) for p in np.unique(self.pen[self.free])]
        offers = {0: self.neighbour_or(seen)} if seed.any() else {}                           # level -> what its set offers
        level = 0
        while offers:
            level += 1
            cand = opened & ~seen
            new = np.zeros_like(seen)
            for w, rows in rows_of:
                for p, of_pen in pens:
                    m = offers.get(level - w - p)
                    if m is None:
                        continue
                    at = np.flatnonzero(m.any(0) & cand.any(0) & of_pen)
                    if len(at):
                        new[:, at] |= self.pack(((m[:, at, None] & rows[:, None, :]) != 0).any(0))
            new &= cand
            at = np.flatnonzero(new.any(0))
            if len(at):
                rr, kk = np.nonzero(self.unpack(new[:, at]))
                state[at[rr], kk] = level
                seen |= new
                offers[level] = self.neighbour_or(new)
            offers.pop(level - self.R + 1, None)      # the largest step is R - 1: level + 1 reads nothing older than level - R + 2
        self.max_level = max(self.max_level, int(state.max()))
        reached = (state >= 0).any(1)
        big = np.where(state >= 0, state, np.int32(2 ** 31 - 1)).min(1)
        cost = np.where(reached, big, NONE).astype(np.int32)
        out = (np.ascontiguousarray(state.T), cost)
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        self._fields[key] = out
        return out

    def heap_dist(self, src, pin=-1):
        """an independent check of levels(): Dijkstra with a binary heap over explicit states (v, k); int32 [K, n]"""
        INF = np.int64(2 ** 62)
        dist = np.full((self.n, self.K), INF, np.int64)
        heap = []
        fr = self.base.seed(int(src), int(pin))
        for k in np.flatnonzero(fr[int(src)]):
            dist[src, k] = 0
            heap.append((0, int(src), int(k)))
        while heap:
            dd, v, k = heapq.heappop(heap)
            if dd > dist[v, k]:
                continue
            for nb in GR.neighbours(v, self.dims):
                nd = np.where(self.adj[k] & self.opened[nb], dd + self.step[k] + self.pen[nb], INF)
                better = np.flatnonzero(nd < dist[nb])
                dist[nb, better] = nd[better]
                for k2 in better.tolist():
                    heapq.heappush(heap, (int(nd[k2]), nb, k2))
        return np.where(dist < INF, dist, NONE).astype(np.int32).T

    def dist_to(self, src, pin, tgt, tpin):
        state, cost = self.levels(src, pin)
        return int(cost[tgt] if tpin < 0 else state[tpin, tgt])

    def matrix(self, pts, pins=None):
        """int32 [P, P]: [i, j] = the cost from (pts[i], pins[i]) to pts[j] restricted to pins[j]"""
        pins = [-1] * len(pts) if pins is None else pins
        return np.array([[self.dist_to(s, p, t, tp) for t, tp in zip(pts, pins)] for s, p in zip(pts, pins)], np.int32).reshape(len(pts), len(pts))

    def path(self, start, end, pin_start=-1, pin_end=-1):
        """(D, ids int64, dirs int32) by the walk-back of rule 33, or (-1, None, None)"""
        state, _ = self.levels(start, pin_start)
        D = self.dist_to(start, pin_start, end, pin_end)
        if D < 0:
            return NONE, None, None
        k = int(np.flatnonzero(state[:, end] == D)[0]) if pin_end < 0 else int(pin_end)
        v, L = int(end), D
        ids, ks = [v], [k]
        while L > 0:
            for nb in GR.neighbours(v, self.dims):
                d = state[:, nb].astype(np.int64)
                ok = np.flatnonzero((d >= 0) & self.adj[:, k] & (d + self.step[:, k] + self.pen[v] == L))
                if len(ok):
                    v, k = nb, int(ok[0])
                    L = int(d[k])
                    break
            else:
                raise AssertionError("a state with a distance has a predecessor")
            ids.append(v)
            ks.append(k)
        return D, np.array(ids[::-1], np.int64), np.array(ks[::-1], np.int32)

    def paths(self, starts, ends, pin_start=None, pin_end=None):
        """(cost int32 [P], [ids or None], [dirs or None])"""
        ps = [-1] * len(starts) if pin_start is None else pin_start
        pe = [-1] * len(starts) if pin_end is None else pin_end
        res = [self.path(int(s), int(e), int(a), int(b)) for s, e, a, b in zip(starts, ends, ps, pe)]
        return np.array([r[0] for r in res], np.int32), [r[1] for r in res], [r[2] for r in res]

    def path_cost(self, ids, ks):
        """the summed step costs of a path"""
        ids, ks = np.asarray(ids, np.int64), np.asarray(ks, np.int64)
        return int((self.step[ks[:-1], ks[1:]] + self.pen[ids[1:]]).sum())

    def check_path(self, ids, ks, start, end, pin_start, pin_end, D):
        """what a path must satisfy whichever rule picked it: pose_ref.Scene.check_path's conditions, and its step costs sum to D"""
        self.base.check_path(ids, ks, start, end, pin_start, pin_end, len(ids) - 1)
        assert self.path_cost(ids, ks) == D


def path_facts(dirs, ids, ks):
    """(hops, direction changes, the sum of U over the steps) of one (voxel, direction) path"""
    q = TR.quantise_all(dirs)
    ks = np.asarray(ks, np.int64)
    U = TR.turn(q[ks[:-1]], q[ks[1:]])
    return len(ids) - 1, int((ks[:-1] != ks[1:]).sum()), int(U.sum())
