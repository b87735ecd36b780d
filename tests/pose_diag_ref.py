"""numpy restatement of the diagonal pose paths of include/weldacs.h (wa_grid_pose_diag_fields, _matrix, _paths; rules 43 - 47 of the
torch section), written from the header's definition and independent of the kernels.  The states, seeds and adjacency are
pose_ref.Scene's.  A face move (v, k) -> (v', k') costs step[0] + turn_costs[class(k, k')] + pen[v']; an edge or corner move keeps the
direction, exists iff k is open in all 2^c voxels of the box the two voxels span, and costs step[c - 1] + pen[v'].  levels() is
level-synchronous on packed masks with the level the distance, like pose_weighted_ref.Scene.levels; heap_dist() is the independent
check, a binary heap over explicit states with the box rule on unpacked booleans; check_path() tests every move voxel by voxel."""
import heapq

import numpy as np

import chamfer_ref as CR
import geodesic_ref as GR
import pose_ref as PR
import pose_weighted_ref as PW

NONE = -1            # WA_DIST_NONE
STEP_MAX = 16
FACES, DIAGS = CR.OFFSETS[:6], CR.OFFSETS[6:]          # (dx, dy, dz); the diagonals in the walk-back's order: 12 edges, 8 corners
CLS = lambda o: sum(1 for c in o if c)   # noqa: E731


class Costs:
    """rule 43: step[3] each 1 .. 16, bands / turn_costs / pen as pose_weighted_ref.Costs"""

    def __init__(self, step, bands=(), turn_costs=(0,), pen=None):
        self.step, self.bands, self.turn_costs = [int(s) for s in step], [int(b) for b in bands], [int(c) for c in turn_costs]
        self.pen = None if pen is None else np.asarray(pen, np.uint8).ravel()
        self.hop = self.step[0]          # what the face moves cost: pose_weighted_ref.Scene reads it
        assert len(self.step) == 3 and all(1 <= s <= STEP_MAX for s in self.step)
        assert len(self.bands) <= PW.MAX_BANDS and len(self.turn_costs) == len(self.bands) + 1
        assert all(0 <= b <= PR.MAX_TURN for b in self.bands) and all(a < b for a, b in zip(self.bands, self.bands[1:]))
        assert self.turn_costs[0] == 0 and max(self.turn_costs) <= PW.COST_MAX
        assert all(a <= b for a, b in zip(self.turn_costs, self.turn_costs[1:]))

    def scaled(self, f):
        return Costs([s * f for s in self.step], self.bands, [c * f for c in self.turn_costs], None if self.pen is None else self.pen * f)


def box(o):
    """the offsets of the 2^c voxels of the box that v and v + o span, relative to v"""
    return [(ax, ay, az) for ax in sorted({0, o[0]}) for ay in sorted({0, o[1]}) for az in sorted({0, o[2]})]


class Scene(PW.Scene):
    """what every search of one (grid, dirs, tool, max_turn, costs) shares.  pose_weighted_ref.Scene gives open, adj, pen, the turn
    classes, the face weights and the packing; R and the diagonal moves are this rule's."""

    def __init__(self, grid, dirs, tool, max_turn, costs, base=None):
        super().__init__(grid, dirs, tool, max_turn, costs, base)
        self.steps = list(costs.step)
        self.R = max(costs.step[0] + max(costs.turn_costs), costs.step[1], costs.step[2]) + self.P + 1
        self._box_open = None
        self._move_ok = None

    def shift(self, words, o):
        """uint64 [W, n] -> b[:, v] = words[:, v + o], 0 where v + o lies outside the grid"""
        nx, ny, nz = self.dims
        dx, dy, dz = o
        a = words.reshape(-1, nz, ny, nx)
        b = np.zeros_like(a)
        zs, zd = slice(max(dz, 0), nz + min(dz, 0)), slice(max(-dz, 0), nz + min(-dz, 0))
        ys, yd = slice(max(dy, 0), ny + min(dy, 0)), slice(max(-dy, 0), ny + min(-dy, 0))
        xs, xd = slice(max(dx, 0), nx + min(dx, 0)), slice(max(-dx, 0), nx + min(-dx, 0))
        b[:, zd, yd, xd] = a[:, zs, ys, xs]
        return b.reshape(len(words), -1)

    def box_open(self):
        """per diagonal offset o, uint64 [W, n]: the directions open in every voxel of the box of v and v + o (0 where the box leaves
        the grid)"""
        if self._box_open is None:
            opened = self.pack(self.opened)
            out = []
            for o in DIAGS:
                m = opened.copy()
                for a in box(o):
                    m &= self.shift(opened, a)
                out.append(m)
            self._box_open = out
        return self._box_open

    def levels(self, src, pin=-1):
        """(state int32 [K, n]: dist(s; v, k) at [k, v], cost int32 [n]) of the source (src, pin); kept, and never modified.  The sets of
        the last R - 1 levels are kept: whole for the diagonal pulls, and as what they offer their six neighbours for the face pulls."""
        key = (int(src), int(pin))
        if key in self._fields:
            return self._fields[key]
        seed = self.base.seed(int(src), int(pin))
        state = np.full((self.n, self.K), NONE, np.int32)
        state[seed] = 0
        opened, seen = self.pack(self.opened), self.pack(seed)
        rows_of = [(w, self.pack(self.adj & (self.step == w))) for w in self.weights]      # [W, K]: who reaches k with a face step of w
        pens = [(int(p), self.pen == p) for p in np.unique(self.pen[self.free])]
        boxes = self.box_open()
        sets = {0: seen.copy()} if seed.any() else {}                                      # level -> its settled set
        offers = {0: self.neighbour_or(seen)} if seed.any() else {}
        level = 0
        while sets:
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
            for c in (2, 3):
                for p, of_pen in pens:
                    S = sets.get(level - self.steps[c - 1] - p)
                    if S is None:
                        continue
                    for o, bx in zip(DIAGS, boxes):
                        if CLS(o) == c:
                            new |= np.where(of_pen[None, :], self.shift(S, o) & bx, np.uint64(0))
            new &= cand
            at = np.flatnonzero(new.any(0))
            if len(at):
                rr, kk = np.nonzero(self.unpack(new[:, at]))
                state[at[rr], kk] = level
                seen |= new
                sets[level] = new
                offers[level] = self.neighbour_or(new)
            sets.pop(level - self.R + 1, None)      # the largest step is R - 1: level + 1 reads nothing older than level - R + 2
            offers.pop(level - self.R + 1, None)
        self.max_level = max(self.max_level, int(state.max()))
        reached = (state >= 0).any(1)
        big = np.where(state >= 0, state, np.int32(2 ** 31 - 1)).min(1)
        cost = np.where(reached, big, NONE).astype(np.int32)
        out = (np.ascontiguousarray(state.T), cost)
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        self._fields[key] = out
        return out

    def move_ok(self):
        """per diagonal offset (flat offset, class, bool [n, K]): the move (v, k) -> (v + o, k) exists, on unpacked booleans"""
        if self._move_ok is None:
            nx, ny, nz = self.dims
            o4 = self.opened.reshape(nz, ny, nx, self.K)
            out = []
            for o in DIAGS:
                ok = np.ones_like(o4)
                for ax, ay, az in box(o):
                    sh = np.zeros_like(o4)
                    zs, zd = slice(max(az, 0), nz + min(az, 0)), slice(max(-az, 0), nz + min(-az, 0))
                    ys, yd = slice(max(ay, 0), ny + min(ay, 0)), slice(max(-ay, 0), ny + min(-ay, 0))
                    xs, xd = slice(max(ax, 0), nx + min(ax, 0)), slice(max(-ax, 0), nx + min(-ax, 0))
                    sh[zd, yd, xd] = o4[zs, ys, xs]
                    ok &= sh
                out.append((o[0] + nx * (o[1] + ny * o[2]), CLS(o), ok.reshape(self.n, self.K)))
            self._move_ok = out
        return self._move_ok

    def heap_dist(self, src, pin=-1):
        """an independent check of levels(): Dijkstra with a binary heap over explicit states (v, k); int32 [K, n]"""
        INF = np.int64(2 ** 62)
        dist = np.full((self.n, self.K), INF, np.int64)
        heap = []
        fr = self.base.seed(int(src), int(pin))
        for k in np.flatnonzero(fr[int(src)]):
            dist[src, k] = 0
            heap.append((0, int(src), int(k)))
        moves = self.move_ok()
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
            for flat, c, ok in moves:
                if ok[v, k]:
                    nb = v + flat
                    nd = dd + self.steps[c - 1] + int(self.pen[nb])
                    if nd < dist[nb, k]:
                        dist[nb, k] = nd
                        heapq.heappush(heap, (int(nd), nb, k))
        return np.where(dist < INF, dist, NONE).astype(np.int32).T

    def coords(self, v):
        nx, ny, _ = self.dims
        return v % nx, (v // nx) % ny, v // (nx * ny)

    def diag_exists(self, v, o, k):
        """the definition, voxel by voxel: every voxel of the box of v and v + o is inside the grid and has k open"""
        nx, ny, nz = self.dims
        x, y, z = self.coords(v)
        for ax, ay, az in box(o):
            qx, qy, qz = x + ax, y + ay, z + az
            if not (0 <= qx < nx and 0 <= qy < ny and 0 <= qz < nz) or not self.opened[qx + nx * (qy + ny * qz), k]:
                return False
        return True

    def path(self, start, end, pin_start=-1, pin_end=-1):
        """(D, ids int64, dirs int32) by the walk-back of rule 44, or (-1, None, None)"""
        state, _ = self.levels(start, pin_start)
        D = self.dist_to(start, pin_start, end, pin_end)
        if D < 0:
            return NONE, None, None
        nx, ny, nz = self.dims
        k = int(np.flatnonzero(state[:, end] == D)[0]) if pin_end < 0 else int(pin_end)
        v, L = int(end), D
        ids, ks = [v], [k]
        while L > 0:
            found = False
            for nb in GR.neighbours(v, self.dims):          # the faces inside the grid, -x, +x, -y, +y, -z, +z
                d = state[:, nb].astype(np.int64)
                ok = np.flatnonzero((d >= 0) & self.adj[:, k] & (d + self.step[:, k] + self.pen[v] == L))
                if len(ok):
                    v, k = nb, int(ok[0])
                    L = int(d[k])
                    found = True
                    break
            if not found:
                x, y, z = self.coords(v)
                for o in DIAGS:
                    want = L - self.steps[CLS(o) - 1] - int(self.pen[v])
                    qx, qy, qz = x + o[0], y + o[1], z + o[2]
                    if want < 0 or not (0 <= qx < nx and 0 <= qy < ny and 0 <= qz < nz):
                        continue
                    q = qx + nx * (qy + ny * qz)
                    if state[k, q] == want and self.diag_exists(v, o, k):
                        v, L = q, want
                        found = True
                        break
            assert found, "a state with a distance has a predecessor"
            ids.append(v)
            ks.append(k)
        return D, np.array(ids[::-1], np.int64), np.array(ks[::-1], np.int32)

    def move_class(self, a, b):
        """the class of the move between two voxels, 0 when they are no 26-neighbours"""
        ca, cb = self.coords(int(a)), self.coords(int(b))
        d = [abs(p - q) for p, q in zip(ca, cb)]
        return sum(d) if max(d) == 1 else 0

    def moves_by_class(self, ids):
        out = [0, 0, 0]
        for a, b in zip(ids[:-1], ids[1:]):
            out[self.move_class(a, b) - 1] += 1
        return out

    def path_cost(self, ids, ks):
        """the summed move costs of a path"""
        total = 0
        for a, b, ka, kb in zip(ids[:-1], ids[1:], ks[:-1], ks[1:]):
            c = self.move_class(a, b)
            total += (int(self.step[ka, kb]) if c == 1 else self.steps[c - 1]) + int(self.pen[b])
        return total

    def check_path(self, ids, ks, start, end, pin_start, pin_end, D):
        """what a path must satisfy whichever rule picked it: it runs from start to end with the pinned directions, every state is open,
        every move is a legal move of its class, and the move costs sum to D"""
        ids, ks = np.asarray(ids, np.int64), np.asarray(ks, np.int64)
        assert len(ids) == len(ks) >= 1 and ids[0] == start and ids[-1] == end
        assert pin_start < 0 or ks[0] == pin_start
        assert pin_end < 0 or ks[-1] == pin_end
        assert self.opened[ids, ks].all()
        for a, b, ka, kb in zip(ids[:-1].tolist(), ids[1:].tolist(), ks[:-1].tolist(), ks[1:].tolist()):
            c = self.move_class(a, b)
            assert c in (1, 2, 3), (a, b)
            if c == 1:
                assert self.adj[ka, kb], (a, b, ka, kb)
            else:
                ca, cb = self.coords(a), self.coords(b)
                assert ka == kb and self.diag_exists(a, tuple(q - p for p, q in zip(ca, cb)), ka), (a, b, ka, kb)
        assert self.path_cost(ids, ks) == D
