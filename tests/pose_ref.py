"""numpy restatement of the exact pose paths of include/weldacs.h (wa_grid_pose_fields, wa_grid_pose_matrix, wa_grid_pose_paths; rules
17 - 23 of the torch section), written from the header's definition and independent of the kernels: a breadth-first search over the
states (voxel, direction) with open(v, k), a step being a 6-neighbour move with a turn of at most max_turn.  Built on
reach_ref.open_dirs, torch_ref.quantise_all and torch_ref.turn.  grid = (free, d2, dims, axes) as torch_ref.make_grid returns it."""
from collections import deque

import numpy as np

import geodesic_ref as GR
import reach_ref as RR
import torch_ref as TR

NONE = -1            # WA_HOPS_NONE
MAX_TURN = 3 << 20   # the largest U there is


def adjacency(dirs, max_turn):
    """adj(k, k') as bool [K, K] (rule 17): everything when max_turn < 0"""
    assert max_turn == -1 or 0 <= max_turn <= MAX_TURN
    q = TR.quantise_all(dirs)
    if max_turn < 0:
        return np.ones((len(q), len(q)), bool)
    return TR.turn(q[:, None, :], q[None, :, :]) <= max_turn


class Scene:
    """what every search of one (grid, dirs, tool, max_turn) shares: open(v, k) and adj"""

    def __init__(self, grid, dirs, tool, max_turn, opened=None):
        self.grid, self.dirs, self.tool, self.max_turn = grid, np.asarray(dirs, np.float32).reshape(-1, 3), tool, max_turn
        self.free = np.asarray(grid[0]).ravel() != 0
        self.dims = grid[2]
        self.opened = RR.open_dirs(grid, self.dirs, tool) if opened is None else opened      # n, K
        self.adj = adjacency(self.dirs, max_turn)
        self.n, self.K = self.opened.shape
        self._fields = {}

    def with_turn(self, max_turn):
        return Scene(self.grid, self.dirs, self.tool, max_turn, self.opened)

    def seed(self, src, pin):
        assert 0 <= src < self.n and self.free[src], "a source on an occupied voxel is an argument error"
        assert -1 <= pin < self.K
        fr = np.zeros((self.n, self.K), bool)
        if pin < 0:
            fr[src] = self.opened[src]
        else:
            fr[src, pin] = self.opened[src, pin]
        return fr

    def levels(self, src, pin=-1):
        """(state int32 [K, n]: level(s; v, k) at [k, v], hops int32 [n]) of the source (src, pin); kept, and never modified"""
        key = (int(src), int(pin))
        if key in self._fields:
            return self._fields[key]
        nx, ny, nz = self.dims
        K = self.K
        fr = self.seed(int(src), int(pin))
        seen = fr.copy()
        state = np.full((self.n, K), NONE, np.int32)
        state[fr] = 0
        adj = self.adj.astype(np.float32)
        level = 0
        while fr.any():
            level += 1
            f = fr.reshape(nz, ny, nx, K)
            m = np.zeros_like(f)
            m[:, :, 1:] |= f[:, :, :-1]
            m[:, :, :-1] |= f[:, :, 1:]
            m[:, 1:] |= f[:, :-1]
            m[:, :-1] |= f[:, 1:]
            m[1:] |= f[:-1]
            m[:-1] |= f[1:]
            m = m.reshape(self.n, K)
            rows = np.flatnonzero(m.any(1))
            fr = np.zeros_like(fr)
            fr[rows] = (m[rows].astype(np.float32) @ adj > 0) & self.opened[rows] & ~seen[rows]
            state[fr] = level
            seen |= fr
        big = np.where(state >= 0, state, np.int32(2 ** 31 - 1)).min(1)
        hops = np.where(seen.any(1), big, NONE).astype(np.int32)
        out = (np.ascontiguousarray(state.T), hops)
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        self._fields[key] = out
        return out

    def hops_to(self, src, pin, tgt, tpin):
        state, hops = self.levels(src, pin)
        return int(hops[tgt] if tpin < 0 else state[tpin, tgt])

    def matrix(self, pts, pins=None):
        """int32 [P, P]: [i, j] = hops from (pts[i], pins[i]) to pts[j] restricted to pins[j]"""
        pins = [-1] * len(pts) if pins is None else pins
        return np.array([[self.hops_to(s, p, t, tp) for t, tp in zip(pts, pins)] for s, p in zip(pts, pins)], np.int32).reshape(len(pts), len(pts))

    def path(self, start, end, pin_start=-1, pin_end=-1):
        """(hops, ids int64 [hops + 1], dirs int32 [hops + 1]) by the walk-back rule, or (-1, None, None)"""
        state, hops = self.levels(start, pin_start)
        D = self.hops_to(start, pin_start, end, pin_end)
        if D < 0:
            return NONE, None, None
        k = int(np.flatnonzero(state[:, end] == D)[0]) if pin_end < 0 else int(pin_end)
        v = int(end)
        ids, ks = [v], [k]
        for L in range(D, 0, -1):
            for nb in GR.neighbours(v, self.dims):
                ok = np.flatnonzero((state[:, nb] == L - 1) & self.adj[:, k])
                if len(ok):
                    v, k = nb, int(ok[0])
                    break
            else:
                raise AssertionError("a state with a level has a predecessor")
            ids.append(v)
            ks.append(k)
        return D, np.array(ids[::-1], np.int64), np.array(ks[::-1], np.int32)

    def paths(self, starts, ends, pin_start=None, pin_end=None):
        """(hops int32 [P], [ids or None], [dirs or None])"""
        ps = [-1] * len(starts) if pin_start is None else pin_start
        pe = [-1] * len(starts) if pin_end is None else pin_end
        res = [self.path(int(s), int(e), int(a), int(b)) for s, e, a, b in zip(starts, ends, ps, pe)]
        return np.array([r[0] for r in res], np.int32), [r[1] for r in res], [r[2] for r in res]

    def queue_levels(self, src, pin=-1):
        """an independent check of levels(): a plain first-in first-out queue over (v, k) tuples"""
        state = np.full((self.K, self.n), NONE, np.int32)
        q = deque()
        fr = self.seed(int(src), int(pin))
        for k in np.flatnonzero(fr[int(src)]):
            state[k, src] = 0
            q.append((int(src), int(k)))
        while q:
            v, k = q.popleft()
            for nb in GR.neighbours(v, self.dims):
                for k2 in range(self.K):
                    if self.adj[k, k2] and self.opened[nb, k2] and state[k2, nb] < 0:
                        state[k2, nb] = state[k, v] + 1
                        q.append((nb, k2))
        return state

    def check_path(self, ids, ks, start, end, pin_start, pin_end, hops):
        """what a path must satisfy whichever rule picked it"""
        q = TR.quantise_all(self.dirs)
        assert len(ids) == len(ks) == hops + 1 and ids[0] == start and ids[-1] == end
        assert pin_start < 0 or ks[0] == pin_start
        assert pin_end < 0 or ks[-1] == pin_end
        assert self.opened[ids, ks].all()
        for a, b in zip(ids[:-1].tolist(), ids[1:].tolist()):
            assert b in GR.neighbours(a, self.dims), (a, b)
        if self.max_turn >= 0 and len(ks) > 1:
            assert (TR.turn(q[ks[:-1]], q[ks[1:]]) <= self.max_turn).all()


def pillars(gap):
    """two pillars with a pocket each, facing one another across `gap` free voxels: grid (12 + gap) x 21 x 21, metal at x 0 .. 5 and
    x 6 + gap .. 11 + gap for y, z 7 .. 13, a 3 x 3 pocket (y, z 9 .. 11) at x 2 .. 5 and x 6 + gap .. 9 + gap; start (3, 10, 10), end
    (8 + gap, 10, 10); 130 directions spread over a cone of half angle 3.1 around +x, a 6-bead rod of 6 voxels.
    dict(grid, dirs, tool, start, end)"""
    nx, ny, nz = 12 + gap, 21, 21
    free = np.ones((nz, ny, nx), np.uint8)
    free[7:14, 7:14, 0:6] = 0
    free[7:14, 7:14, 6 + gap:12 + gap] = 0
    free[9:12, 9:12, 2:6] = 1
    free[9:12, 9:12, 6 + gap:10 + gap] = 1
    idx = lambda x, y, z: (z * ny + y) * nx + x   # noqa: E731
    return dict(grid=TR.make_grid(free, (nx, ny, nz)), dirs=TR.fib_dirs(130, 3.1, (1.0, 0.0, 0.0)), tool=TR.rod(6, 96, 1),
                start=idx(3, 10, 10), end=idx(8 + gap, 10, 10))


def wide_scene():
    """70 x 9 x 7 with three boxes: x crosses a wavefront's 64 lanes with a tail of 6, ny * nz = 63 rows; 33 directions in a cone of half
    angle 1.2 around +z, a 4-bead rod of 3 voxels.  dict(grid, dirs, tool, points)"""
    nx, ny, nz = 70, 9, 7
    free = np.ones((nz, ny, nx), np.uint8)
    free[0:4, 2:6, 20:24] = 0
    free[3:7, 0:5, 60:66] = 0
    free[0:5, 4:9, 40:43] = 0
    idx = lambda x, y, z: (z * ny + y) * nx + x   # noqa: E731
    pts = [idx(0, 0, 0), idx(69, 8, 6), idx(63, 4, 1), idx(64, 6, 5), idx(30, 3, 0), idx(67, 2, 2)]
    return dict(grid=TR.make_grid(free, (nx, ny, nz)), dirs=TR.fib_dirs(33, 1.2, (0.0, 0.0, 1.0)), tool=TR.rod(4, 48, 1), points=pts)


def spread_points(grid, count):
    """`count` free voxels spread evenly over the free voxels in raster order"""
    f = np.flatnonzero(np.asarray(grid[0]).ravel() != 0)
    return [int(f[i]) for i in np.linspace(0, len(f) - 1, count).astype(np.int64)]


BOX_TURNS = (250000, 0, 250000, 0)   # max_turn of box_case(seed)


def box_case(seed):
    """reach_ref.box_scene(seed) at 24^3 with six points, the first, third and fifth pinned"""
    grid, dirs, tool = RR.box_scene(seed, 24)
    K = len(dirs)
    return dict(grid=grid, dirs=dirs, tool=tool, max_turn=BOX_TURNS[seed], points=spread_points(grid, 6), pins=[0, -1, K - 1, -1, 1, -1])


def tunnel_case():
    """reach_ref.tunnel_scene() with a turn limit and the start pinned: start and end stay connected, more than 64 levels"""
    t = RR.tunnel_scene()
    idx = lambda x, y, z: (z * 24 + y) * 40 + x   # noqa: E731
    return dict(grid=t["grid"], dirs=t["dirs"], tool=t["tool"], max_turn=8000, points=[t["start"], t["end"], idx(20, 11, 3), idx(39, 23, 27)],
                pins=[31, -1, -1, 3])


def wide_case():
    w = wide_scene()
    return dict(grid=w["grid"], dirs=w["dirs"], tool=w["tool"], max_turn=30000, points=w["points"], pins=[32, -1, -1, 0, -1, 7])


def first_field_facts(case):
    """of the search from the case's first point with its pin: (open states never reached, voxels the fit grid reaches sooner or that
    are not reached at all, the deepest level, hops to every point)"""
    sc = Scene(case["grid"], case["dirs"], case["tool"], case["max_turn"])
    src, pin = case["points"][0], case["pins"][0]
    state, hops = sc.levels(src, pin)
    fit = RR.fit(case["grid"], case["dirs"], case["tool"], 1, count=sc.opened.sum(1))
    gh = GR.field(fit, sc.dims, src)
    unreached = int(((state < 0).T & sc.opened).sum())
    later = int(((gh >= 0) & ((hops > gh) | (hops < 0))).sum())
    return unreached, later, int(state.max()), hops[case["points"]]
