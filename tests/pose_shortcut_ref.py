"""numpy restatement of wa_grid_pose_shortcut (include/weldacs.h, rules 27 - 29 of the torch section), written from the header's
definition and independent of the kernels: the greedy any-angle shortcut of (voxel, direction) paths whose candidates must keep one
of the two end directions open in every voxel of the supercover.  Built on reach_ref.open_dirs, torch_ref.quantise_all,
torch_ref.turn and clearance_ref.supercover; the length is shortcut_ref.length.  grid = (free, d2, dims, axes) as torch_ref.make_grid
returns it."""
import numpy as np

import clearance_ref as CR
import pose_ref as PR
import reach_ref as RR
import shortcut_ref as SR
import torch_ref as TR

SUMMARY_FIELDS = ("n_paths", "n_nodes", "n_waypoints", "n_held_start", "n_held_end", "n_unheld", "max_hold_turn")


class Scene:
    """what every path of one (grid, dirs, tool, max_turn) shares: open(v, k), adj, the quantised directions and a cache of covers"""

    def __init__(self, grid, dirs, tool, max_turn, opened=None):
        self.grid, self.dirs, self.tool, self.max_turn = grid, np.asarray(dirs, np.float32).reshape(-1, 3), tool, max_turn
        self.dims = grid[2]
        self.opened = RR.open_dirs(grid, self.dirs, tool) if opened is None else opened      # n, K
        self.n, self.K = self.opened.shape
        self.q = TR.quantise_all(self.dirs)
        self.adj = PR.adjacency(self.dirs, max_turn)
        self._covers = {}

    def with_turn(self, max_turn):
        return Scene(self.grid, self.dirs, self.tool, max_turn, self.opened)

    def cover(self, va, vm):
        """raster ids of the supercover between voxels va and vm (ids), voxel va included"""
        key = (int(va), int(vm))
        if key not in self._covers:
            nx, ny, _ = self.dims
            self._covers[key] = np.array([(z * ny + y) * nx + x for x, y, z in CR.supercover(SR.voxel(va, nx, ny), SR.voxel(vm, nx, ny))],
                                         np.int64)
        return self._covers[key]

    def cover_open(self, va, vm, k):
        return bool(self.opened[self.cover(va, vm), int(k)].all())

    def ok(self, va, ka, vm, km):
        return bool(self.adj[ka, km]) and (self.cover_open(va, vm, ka) or self.cover_open(va, vm, km))

    def hold(self, va, ka, vj, kj):
        """rule 28: -1 without ok, else k_a if its cover is open, else k_j"""
        if not self.ok(va, ka, vj, kj):
            return -1
        return int(ka) if self.cover_open(va, vj, ka) else int(kj)

    def shortcut(self, ids, ks, max_span):
        """(waypoint indices int64, holds int32 of the same length with a last entry of -1, float64 length) of one path"""
        assert 1 <= max_span <= 4096
        ids, ks = np.asarray(ids, np.int64).reshape(-1), np.asarray(ks, np.int64).reshape(-1)
        assert len(ids) == len(ks) and (len(ks) == 0 or (ks.min() >= 0 and ks.max() < self.K))
        L = len(ids)
        if L == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int32), 0.0
        wp, holds = [0], []
        a = 0
        while a < L - 1:
            j = a
            for m in range(a + 1, min(a + max_span, L - 1) + 1):      # prefix form: stop at the first candidate without ok
                if not self.ok(ids[a], ks[a], ids[m], ks[m]):
                    break
                j = m
            j = j if j > a else a + 1
            holds.append(self.hold(ids[a], ks[a], ids[j], ks[j]))
            wp.append(j)
            a = j
        holds.append(-1)
        nx, ny, _ = self.dims
        w = np.asarray(wp, np.int64)
        return w, np.asarray(holds, np.int32), SR.length(ids[w], nx, ny, *self.grid[3])

    def batch(self, paths, kss, max_span):
        """([waypoint indices], [holds], float64 lengths, summary dict) of a batch"""
        res = [self.shortcut(p, k, max_span) for p, k in zip(paths, kss)]
        s = dict.fromkeys(SUMMARY_FIELDS, 0)
        s["n_paths"] = len(res)
        s["n_nodes"] = int(sum(len(p) for p in paths))
        for (w, h, _), k in zip(res, kss):
            k = np.asarray(k, np.int64).reshape(-1)
            s["n_waypoints"] += len(w)
            seg = h[:-1].astype(np.int64) if len(h) else np.zeros(0, np.int64)
            ka = k[w[:-1]] if len(w) else np.zeros(0, np.int64)
            s["n_unheld"] += int((seg < 0).sum())
            s["n_held_start"] += int(((seg >= 0) & (seg == ka)).sum())
            s["n_held_end"] += int(((seg >= 0) & (seg != ka)).sum())
            for h0, h1 in zip(seg[:-1], seg[1:]):
                if h0 >= 0 and h1 >= 0:
                    s["max_hold_turn"] = max(s["max_hold_turn"], int(TR.turn(self.q[h0], self.q[h1])))
        return [r[0] for r in res], [r[1] for r in res], np.array([r[2] for r in res], np.float64), s


def point_tool():
    """identity (a): one bead on the tip with r2 = 0, blocked only on an occupied voxel"""
    return np.zeros(1, np.int64), np.zeros(1, np.int64)


def scene_paths():
    """the pose paths of the issue's scenes, planned by pose_ref: {name: dict(grid, dirs, tool, max_turn, ids, ks)}; computed once"""
    if not _SCENES:
        for gap in (4, 6):
            p = PR.pillars(gap)
            sc = PR.Scene(p["grid"], p["dirs"], p["tool"], 150000)
            _, ids, ks = sc.path(p["start"], p["end"])
            _SCENES["pillars%d" % gap] = dict(grid=p["grid"], dirs=p["dirs"], tool=p["tool"], max_turn=150000, ids=ids, ks=ks, opened=sc.opened)
        w = PR.wide_case()
        sc = PR.Scene(w["grid"], w["dirs"], w["tool"], w["max_turn"])
        _, ids, ks = sc.path(w["points"][4], w["points"][5], -1, 7)
        _SCENES["wide"] = dict(grid=w["grid"], dirs=w["dirs"], tool=w["tool"], max_turn=w["max_turn"], ids=ids, ks=ks, opened=sc.opened)
    return _SCENES


_SCENES = {}


def wide_row(closed=False):
    """hand-made paths on pose_ref.wide_scene(): the 70 nodes of the row y = 0, z = 0 with ONE direction for all of them -- the lowest
    that is open on every node, or (closed) the one that is closed on the fewest interior nodes of the row, but on one at least.
    dict(grid, dirs, tool, ids, ks, opened)"""
    w = PR.wide_scene()
    opened = RR.open_dirs(w["grid"], w["dirs"], w["tool"])
    ids = np.arange(70, dtype=np.int64)
    shut = (~opened[ids[1:-1]]).sum(0)                  # K
    if closed:
        k = int(np.flatnonzero(shut == shut[shut > 0].min())[0])
    else:
        k = int(np.flatnonzero((shut == 0) & opened[0] & opened[69])[0])
    return dict(grid=w["grid"], dirs=w["dirs"], tool=w["tool"], ids=ids, ks=np.full(70, k, np.int32), opened=opened)


def lowest_open(opened, ids):
    """per node the lowest open direction of its voxel, 0 where none is open"""
    o = opened[np.asarray(ids, np.int64)]
    return np.where(o.any(1), o.argmax(1), 0).astype(np.int32)
