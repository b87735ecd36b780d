"""Thin numpy-facing wrappers over the C ABI (include/weldacs.h) for tests and bench.py.
All compute happens in libweldacs.so's HIP kernels; this file only marshals pointers."""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _lib as L
from ._lib import AcsParams, GtspParams, RNG_DEV, RNG_REF, WA_COST_MAX, WA_D2_NONE, WA_DIST_NONE, WA_HOPS_NONE, WeldacsError  # noqa: F401


RETIME_Q = 1 << 30   # quanta per unit in wa_traj_retime's integers


def _ptr(a):
    return a.ctypes.data if a is not None else None


# Contexts still open when the interpreter exits are closed HERE, children first, while the HIP / RCCL runtimes are still up: left to
# __del__ during interpreter teardown the destroy calls can arrive after those runtimes' own exit handlers have run (seen on ROCm 7.2 as
# "terminate called after throwing std::bad_variant_access" from a communicator destroyed that late).
_live_contexts = weakref.WeakSet()


@atexit.register
def _close_live_contexts():
    for c in list(_live_contexts):
        try:
            c.close()
        except Exception:   # noqa: BLE001 -- exit path: nothing useful can be done with an error here
            pass


class Context:
    def __init__(self, device=0, lib_path=None):
        self.lib = L.load(lib_path)
        h = C.c_void_p()
        rc = self.lib.wa_ctx_create(device, C.byref(h))
        if rc:
            raise WeldacsError(rc, "wa_ctx_create(%d) failed: no usable HIP device" % device)
        self.h = h
        self._children = weakref.WeakSet()  # grids / solvers must be destroyed before the context
        _live_contexts.add(self)

    def check(self, rc):
        if rc:
            raise WeldacsError(rc, self.lib.wa_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            for ch in sorted(list(self._children), key=lambda o: 0 if isinstance(o, (AcsSolver, Comm)) else 1):
                ch.close()
            self.lib.wa_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        self.lib.wa_ctx_device_name(self.h, buf, 256)
        return buf.value.decode()

    @property
    def stream(self):
        return self.lib.wa_ctx_stream(self.h)

    def memory_info(self):
        """(free, total) bytes of device memory"""
        f, t = C.c_int64(), C.c_int64()
        self.check(self.lib.wa_ctx_memory_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def cached_bytes(self):
        """device bytes of destroyed solvers this context keeps for its next solver (wa_ctx_cached_bytes); counted as free by memory_info"""
        b = C.c_int64()
        self.check(self.lib.wa_ctx_cached_bytes(self.h, C.byref(b)))
        return b.value

    def trim(self):
        """give the kept blocks back to the driver (wa_ctx_trim)"""
        self.check(self.lib.wa_ctx_trim(self.h))

    def cache_stats(self):
        """wa_ctx_cache_stats as a dict: what the context's kept memory served and what had to come from the driver"""
        v = (C.c_int64 * 8)()
        self.check(self.lib.wa_ctx_cache_stats(self.h, v))
        keys = ("blocks", "hit_bytes", "miss_bytes", "released_bytes", "blocks_all_from_kept", "oom_events", "arena_build_ms", "arena")
        d = {k: int(x) for k, x in zip(keys, v)}
        d["kept_bytes"] = self.cached_bytes()
        return d

    def poison_stats(self):
        """wa_ctx_poison_stats as a dict: blocks / bytes that WA_DEV_POISON=1 filled, per allocator (all 0 without the knob)"""
        v = (C.c_int64 * 4)()
        self.check(self.lib.wa_ctx_poison_stats(self.h, v))
        return {k: int(x) for k, x in zip(("ctx_blocks", "ctx_bytes", "plain_blocks", "plain_bytes"), v)}

    GUARD_KEYS = ("handed_out", "checked", "live_blocks", "live_bytes", "front_damaged", "back_damaged", "first_bytes", "first_distance")

    def guard_stats(self):
        """wa_ctx_guard_stats as a dict: the red zones of WA_DEV_GUARD=1 -- blocks handed out, freed and checked, live (with their
        requested bytes), freed with a damaged front / back zone, and the first damaged block's size and the distance of its first
        damaged byte (>= 0 behind the block, < 0 in front of it).  All 0, first_bytes -1, without the knob."""
        v = (C.c_int64 * 8)()
        self.check(self.lib.wa_ctx_guard_stats(self.h, v))
        return {k: int(x) for k, x in zip(self.GUARD_KEYS, v)}

    def guard_selftest(self, n_bytes, offset):
        """wa_ctx_guard_selftest: one byte written at `offset` of a guarded block of `n_bytes` that the library allocates and frees"""
        self.check(self.lib.wa_ctx_guard_selftest(self.h, int(n_bytes), int(offset)))

    def sync(self):
        self.check(self.lib.wa_ctx_sync(self.h))


def stl_parse(data):
    lib = L.load()
    buf = np.frombuffer(data, np.uint8)
    n = lib.wa_stl_parse(_ptr(buf), len(buf), None, 0)
    if n < 0:
        raise WeldacsError(-n, "wa_stl_parse")
    tris = np.empty((n, 12), np.float32)
    lib.wa_stl_parse(_ptr(buf), len(buf), _ptr(tris), n)
    return tris


def stl_read_file(path):
    lib = L.load()
    n = lib.wa_stl_read_file(path.encode(), None, 0)
    if n < 0:
        raise WeldacsError(-n, "wa_stl_read_file(%s)" % path)
    tris = np.empty((n, 12), np.float32)
    lib.wa_stl_read_file(path.encode(), _ptr(tris), n)
    return tris


def axis_coords(lo, hi, precision, wall, n):
    out = np.empty(n, np.float32)
    L.load().wa_axis_coords(C.c_float(lo), C.c_float(hi), C.c_float(precision), wall, n, _ptr(out))
    return out


class Grid:
    def __init__(self, ctx, handle, bbox=None):
        self.ctx, self.h, self.bbox = ctx, handle, bbox
        ctx._children.add(self)
        dims = np.zeros(3, np.int32)
        p, w, nf = C.c_float(), C.c_int32(), C.c_int64()
        ctx.check(ctx.lib.wa_grid_info(self.h, _ptr(dims), C.byref(p), C.byref(w), C.byref(nf)))
        self.nx, self.ny, self.nz = (int(v) for v in dims)
        self.precision, self.wall, self.n_free = np.float32(p.value), w.value, nf.value

    @classmethod
    def from_mesh(cls, ctx, tris, precision, wall):
        tris = np.ascontiguousarray(tris, np.float32)
        h = C.c_void_p()
        bbox = np.zeros(6, np.float32)
        ctx.check(ctx.lib.wa_grid_from_mesh(ctx.h, _ptr(tris), len(tris), C.c_float(precision), wall, C.byref(h), _ptr(bbox)))
        return cls(ctx, h, bbox)

    @classmethod
    def from_occupancy(cls, ctx, free, cx, cy, cz, precision, wall=0):
        free = np.ascontiguousarray(free, np.uint8).reshape(-1)
        cx, cy, cz = (np.ascontiguousarray(a, np.float32) for a in (cx, cy, cz))
        assert free.size == len(cx) * len(cy) * len(cz)
        h = C.c_void_p()
        ctx.check(ctx.lib.wa_grid_from_occupancy(ctx.h, _ptr(free), len(cx), len(cy), len(cz), _ptr(cx), _ptr(cy),
                                                 _ptr(cz), C.c_float(precision), wall, C.byref(h)))
        return cls(ctx, h)

    @property
    def n(self):
        return self.nx * self.ny * self.nz

    def occupancy(self):
        out = np.empty(self.n, np.uint8)
        self.ctx.check(self.ctx.lib.wa_grid_read_occupancy(self.h, _ptr(out)))
        return out

    def coords(self):
        cx, cy, cz = np.empty(self.nx, np.float32), np.empty(self.ny, np.float32), np.empty(self.nz, np.float32)
        self.ctx.check(self.ctx.lib.wa_grid_read_coords(self.h, _ptr(cx), _ptr(cy), _ptr(cz)))
        return cx, cy, cz

    def resolve(self, pts):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        ids = np.empty(len(pts), np.int64)
        self.ctx.check(self.ctx.lib.wa_grid_resolve_points(self.h, _ptr(pts), len(pts), _ptr(ids)))
        return ids

    def distance_field(self):
        """exact squared distance to the nearest occupied voxel, in voxel-index units (flat int32, raster order like occupancy();
        WA_D2_NONE everywhere on a grid without obstacles)"""
        out = np.empty(self.n, np.int32)
        self.ctx.check(self.ctx.lib.wa_grid_distance_field(self.h, _ptr(out)))
        return out

    def inflate(self, radius, keep_ids=None):
        """a planning grid whose free voxels lie farther than `radius` voxels from every obstacle, except within radius + 1 of each
        keep id (weld points resolved on this grid), where this grid's state is kept"""
        keep = np.ascontiguousarray(keep_ids if keep_ids is not None else [], np.int64).reshape(-1)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.wa_grid_inflate(self.h, C.c_float(radius), _ptr(keep) if len(keep) else None, len(keep), C.byref(h)))
        return Grid(self.ctx, h, self.bbox)

    def _torch_args(self, dirs, tool):
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        return dirs, len(dirs), tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)

    def torch_reach(self, dirs, tool, masks=True):
        """wa_grid_tool_reach: for every voxel, which of the K directions `dirs` (K x 3, tip -> body) keep the beads of `tool` clear of
        this grid's metal when the tip is on that voxel.  Returns (mask uint64[W, n] or None with masks=False -- bit k & 63 of
        mask[k >> 6, v] is set where direction k is open at v --, count uint16[n], summary dict).  Occupied voxels have no open direction."""
        dirs, K, tool = self._torch_args(dirs, tool)
        mask = np.empty(((K + 63) // 64, self.n), np.uint64) if masks else None
        count = np.empty(self.n, np.uint16)
        s = L.ReachSummary()
        self.ctx.check(self.ctx.lib.wa_grid_tool_reach(self.h, _ptr(dirs), K, C.byref(tool), _ptr(mask), _ptr(count), C.byref(s)))
        return mask, count, {k: int(getattr(s, k)) for k, _ in L.ReachSummary._fields_}

    def torch_fit(self, dirs, tool, min_dirs=1, keep_ids=None, keep_r2=0):
        """wa_grid_tool_fit: a planning grid whose free voxels are this grid's free voxels with at least `min_dirs` open directions,
        except within sqrt(keep_r2) voxels of each keep id (weld points resolved on this grid), where this grid's state is kept.  The
        summary of torch_reach is left in the result's `reach_summary`."""
        dirs, K, tool = self._torch_args(dirs, tool)
        keep = np.ascontiguousarray(keep_ids if keep_ids is not None else [], np.int64).reshape(-1)
        h, s = C.c_void_p(), L.ReachSummary()
        self.ctx.check(self.ctx.lib.wa_grid_tool_fit(self.h, _ptr(dirs), K, C.byref(tool), min_dirs, _ptr(keep) if len(keep) else None,
                                                     len(keep), keep_r2, C.byref(h), C.byref(s)))
        g = Grid(self.ctx, h, self.bbox)
        g.reach_summary = {k: int(getattr(s, k)) for k, _ in L.ReachSummary._fields_}
        return g

    def torch_penalties(self, dirs, tool, thr):
        """wa_grid_tool_penalties: uint8 [n] for chamfer_weighted_*: 0 on occupied voxels, else the number of thresholds in `thr` (at most
        WA_PEN_MAX of them, each 0 .. 65535) that the voxel's count of open directions stays below"""
        dirs, K, tool = self._torch_args(dirs, tool)
        thr = np.ascontiguousarray(thr, np.int32).reshape(-1)
        pen = np.empty(self.n, np.uint8)
        self.ctx.check(self.ctx.lib.wa_grid_tool_penalties(self.h, _ptr(dirs), K, C.byref(tool), _ptr(thr) if len(thr) else None, len(thr),
                                                           _ptr(pen)))
        return pen

    @staticmethod
    def _pins(pins, count, what):
        """a pin array for the pose calls: None stays None (all -1)"""
        if pins is None:
            return None
        pins = np.ascontiguousarray(pins, np.int32).reshape(-1)
        assert len(pins) == count, "one pin per " + what
        return pins

    def _pose_fields(self, fn, lead, ids, pins, states):
        """the marshalling of the three pose _fields calls: fn(grid, *lead, ids, pins, len(ids), out, state), out int32 [len(ids), n],
        state int32 [len(ids), K, n] or NULL; lead = (dirs, K, tool, max_turn[, costs]); empty arrays as in _search_rows"""
        K = lead[1]
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        pins = self._pins(pins, len(ids), "source")
        out = np.empty((len(ids), self.n), np.int32)
        state = np.empty((len(ids), K, self.n), np.int32) if states else None
        pad = np.zeros(1, np.int32)
        self.ctx.check(fn(self.h, *lead, _ptr(ids if len(ids) else np.zeros(1, np.int64)), _ptr(pins) if pins is not None and len(ids) else None,
                          len(ids), _ptr(out if out.size else pad), (_ptr(state if state.size else pad)) if states else None))
        return (out, state) if states else out

    def _pose_matrix(self, fn, lead, ids, pins):
        """the marshalling of the three pose _matrix calls: fn(grid, *lead, ids, pins, len(ids), out), out int32 [len(ids), len(ids)]"""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        pins = self._pins(pins, len(ids), "point")
        out = np.empty((len(ids), len(ids)), np.int32)
        self.ctx.check(fn(self.h, *lead, _ptr(ids if len(ids) else np.zeros(1, np.int64)), _ptr(pins) if pins is not None and len(ids) else None,
                          len(ids), _ptr(out if out.size else np.zeros(1, np.int32))))
        return out

    def _pose_paths(self, fn, lead, starts, ends, pin_start, pin_end):
        """the two calls of the three pose _paths calls: fn is the library's _paths call, lead as for _pose_fields.  The first call, with
        empty ranges, returns the distances and node counts, the second writes the paths into ranges of those counts."""
        starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
        ends = np.ascontiguousarray(ends, np.int64).reshape(-1)
        assert len(starts) == len(ends)
        n = len(starts)
        ps, pe = self._pins(pin_start, n, "pair"), self._pins(pin_end, n, "pair")
        cost, lens = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        off = np.zeros(n + 1, np.int64)
        pad = np.zeros(1, np.int64)

        def call(ids, ks):
            return fn(self.h, *lead, _ptr(starts if n else pad), _ptr(ends if n else pad), _ptr(ps) if ps is not None and n else None,
                      _ptr(pe) if pe is not None and n else None, n, _ptr(off), _ptr(ids), _ptr(ks), _ptr(cost), _ptr(lens))
        rc = call(pad, np.zeros(1, np.int32))
        if rc not in (0, 7):
            self.ctx.check(rc)
        off[1:] = np.cumsum(np.where(cost[:n] >= 0, lens[:n], 0).astype(np.int64))
        ids, ks = np.empty(max(int(off[-1]), 1), np.int64), np.empty(max(int(off[-1]), 1), np.int32)
        if rc == 7:
            self.ctx.check(call(ids, ks))
        cost = cost[:n]
        return (cost, [ids[off[k]:off[k + 1]].copy() if cost[k] >= 0 else None for k in range(n)],
                [ks[off[k]:off[k + 1]].copy() if cost[k] >= 0 else None for k in range(n)])

    def _pose_costs(self, costs, cls, factory):
        """the cost description of a pose call by reference: `costs` is an instance of `cls`, which api.`factory` returns"""
        assert isinstance(costs, cls), "costs come from api." + factory
        assert costs.pen is None or costs.pen.size == self.n, "a penalty array holds one byte per voxel"
        return C.byref(costs.c)

    def pose_fields(self, dirs, tool, max_turn, ids, pins=None, states=False):
        """wa_grid_pose_fields: exact hop counts over the states (voxel, direction) -- a step moves to a 6-neighbour voxel and turns the
        torch by at most `max_turn` (the measure U of torch_axes; -1: no limit), and every state on the way has the direction open.
        `pins`: per source a direction index the search starts with, or -1 for every open one.  Returns int32 hops [len(ids), n], the
        least level over the directions (WA_HOPS_NONE (-1) where no state is reached), and with states=True also int32
        [len(ids), K, n], the level of every state."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn))
        return self._pose_fields(self.ctx.lib.wa_grid_pose_fields, lead, ids, pins, states)

    def pose_matrix(self, dirs, tool, max_turn, ids, pins=None):
        """wa_grid_pose_matrix: int32 [P, P] of those hop counts between the points; a point's pin restricts both the directions it starts
        with as a source and the direction it must be reached with as a target (symmetric; WA_HOPS_NONE (-1) where two points are not
        connected, on the diagonal too when the point has no open direction its pin allows)"""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn))
        return self._pose_matrix(self.ctx.lib.wa_grid_pose_matrix, lead, ids, pins)

    def pose_paths(self, dirs, tool, max_turn, starts, ends, pin_start=None, pin_end=None):
        """wa_grid_pose_paths of a batch of pairs: (int32 hops, [node-id array per pair, start first], [int32 direction index per node]);
        None in both lists where hops is WA_HOPS_NONE.  Two calls: the first, with empty ranges, returns the counts (WA_ERR_CAPACITY is
        its expected status when any pair is reachable), the second writes the paths into ranges of hops + 1."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn))
        return self._pose_paths(self.ctx.lib.wa_grid_pose_paths, lead, starts, ends, pin_start, pin_end)

    def pose_weighted_fields(self, dirs, tool, max_turn, costs, ids, pins=None, states=False):
        """wa_grid_pose_weighted_fields: pose_fields with a price on every step -- `costs` (api.pose_costs) charges a step its hop cost,
        the turn cost of the class its change of direction falls in and the penalty of the voxel it enters.  Returns int32 cost
        [len(ids), n], the least distance over the directions (WA_DIST_NONE (-1) where no state is reached), and with states=True also
        int32 [len(ids), K, n], the distance of every state."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseCosts, "pose_costs"))
        return self._pose_fields(self.ctx.lib.wa_grid_pose_weighted_fields, lead, ids, pins, states)

    def pose_weighted_matrix(self, dirs, tool, max_turn, costs, ids, pins=None):
        """wa_grid_pose_weighted_matrix: int32 [P, P] of those costs between the points, pins as for pose_matrix (symmetric when `costs`
        has no penalties and both sides carry the same pins; WA_DIST_NONE (-1) where two points are not connected)"""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseCosts, "pose_costs"))
        return self._pose_matrix(self.ctx.lib.wa_grid_pose_weighted_matrix, lead, ids, pins)

    def pose_weighted_paths(self, dirs, tool, max_turn, costs, starts, ends, pin_start=None, pin_end=None):
        """wa_grid_pose_weighted_paths of a batch of pairs: (int32 cost, [node-id array per pair, start first], [int32 direction index
        per node]); None in both lists where the cost is WA_DIST_NONE.  The lists feed pose_shortcut_paths as those of pose_paths do.  Two
        calls: the first, with empty ranges, returns the costs and node counts (WA_ERR_CAPACITY is its expected status when any pair is
        reachable), the second writes the paths into ranges of those counts."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseCosts, "pose_costs"))
        return self._pose_paths(self.ctx.lib.wa_grid_pose_weighted_paths, lead, starts, ends, pin_start, pin_end)

    def pose_diag_fields(self, dirs, tool, max_turn, costs, ids, pins=None, states=False):
        """wa_grid_pose_diag_fields: pose_weighted_fields on the 26-neighbour lattice -- `costs` (api.pose_diag_costs) charges a face move
        step[0] plus the turn cost of its change of direction, an edge or corner move step[1] or step[2]; a diagonal move keeps the
        direction and needs it open in every voxel of the box it spans; every move pays the penalty of the voxel it enters.  Returns
        int32 cost [len(ids), n] (WA_DIST_NONE (-1) where no state is reached), and with states=True also int32 [len(ids), K, n], the
        distance of every state."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseDiagCosts, "pose_diag_costs"))
        return self._pose_fields(self.ctx.lib.wa_grid_pose_diag_fields, lead, ids, pins, states)

    def pose_diag_matrix(self, dirs, tool, max_turn, costs, ids, pins=None):
        """wa_grid_pose_diag_matrix: int32 [P, P] of those costs between the points, pins as for pose_matrix (symmetric when `costs` has
        no penalties and both sides carry the same pins; WA_DIST_NONE (-1) where two points are not connected)"""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseDiagCosts, "pose_diag_costs"))
        return self._pose_matrix(self.ctx.lib.wa_grid_pose_diag_matrix, lead, ids, pins)

    def pose_diag_paths(self, dirs, tool, max_turn, costs, starts, ends, pin_start=None, pin_end=None):
        """wa_grid_pose_diag_paths of a batch of pairs, returned as pose_weighted_paths returns its paths (and by the same two calls):
        consecutive nodes are 26-neighbours, and the direction index changes on face moves only.  The lists feed pose_shortcut_paths."""
        dirs, K, tool = self._torch_args(dirs, tool)
        lead = (_ptr(dirs), K, C.byref(tool), int(max_turn), self._pose_costs(costs, PoseDiagCosts, "pose_diag_costs"))
        return self._pose_paths(self.ctx.lib.wa_grid_pose_diag_paths, lead, starts, ends, pin_start, pin_end)

    def clearance_radius(self, metres):
        """a clearance in metres as a radius in voxels (exact up to the hi-side seam of the wall, see include/weldacs.h)"""
        return float(metres) / float(self.precision)

    def shortcut(self, path, max_span=128):
        """wa_grid_path_shortcut of one path: (waypoint node ids, shortened length in metres)"""
        wps, lengths = shortcut_paths(self, [path], max_span)
        return wps[0], float(lengths[0])

    def _search_rows(self, fn, lead, ids, points):
        """the marshalling of the four fields / matrix calls: fn(grid, *lead, ids, len(ids), out), out int32 [len(ids), n] or, points,
        [len(ids), len(ids)]; an empty array is passed as a one-element stand-in (the C side wants pointers that are not NULL)"""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        out = np.empty((len(ids), len(ids) if points else self.n), np.int32)
        self.ctx.check(fn(self.h, *lead, _ptr(ids if len(ids) else np.zeros(1, np.int64)), len(ids), _ptr(out if out.size else np.zeros(1, np.int32))))
        return out

    def geodesic_fields(self, ids):
        """wa_grid_geodesic_fields: int32 [len(ids), n], exact hop counts on the 6-neighbour lattice of free voxels from each source
        (free voxels) to every voxel; WA_HOPS_NONE (-1) where there is no path"""
        return self._search_rows(self.ctx.lib.wa_grid_geodesic_fields, (), ids, False)

    def geodesic_matrix(self, ids):
        """wa_grid_geodesic_matrix: int32 [P, P] hop counts between the points (symmetric, 0 on the diagonal, WA_HOPS_NONE (-1) where
        two points are not connected)"""
        return self._search_rows(self.ctx.lib.wa_grid_geodesic_matrix, (), ids, True)

    def clearance_costs(self, thr2):
        """wa_grid_clearance_costs: uint8 [n], 0 on occupied voxels, else 1 + the number of thresholds (squared distances in voxels, at
        most WA_COST_MAX - 1 of them) that the voxel's entry in distance_field() does not exceed"""
        thr2 = np.ascontiguousarray(thr2, np.int32).reshape(-1)
        out = np.empty(self.n, np.uint8)
        self.ctx.check(self.ctx.lib.wa_grid_clearance_costs(self.h, _ptr(thr2 if len(thr2) else np.zeros(1, np.int32)), len(thr2), _ptr(out)))
        return out

    def _cost(self, cost):
        cost = np.ascontiguousarray(cost, np.uint8).reshape(-1)
        assert cost.size == self.n, "a cost array holds one byte per voxel"
        return cost

    def weighted_fields(self, cost, ids):
        """wa_grid_weighted_fields: int32 [len(ids), n], the exact least sum of entry costs (cost: uint8 [n], 1 .. WA_COST_MAX on free
        voxels) from each source to every voxel; WA_DIST_NONE (-1) where there is no path"""
        cost = self._cost(cost)
        return self._search_rows(self.ctx.lib.wa_grid_weighted_fields, (_ptr(cost),), ids, False)

    def weighted_matrix(self, cost, ids):
        """wa_grid_weighted_matrix: int32 [P, P], [i, j] = dist(point i, point j) (not symmetric: [i, j] - [j, i] = cost[j] - cost[i]);
        WA_DIST_NONE (-1) where two points are not connected"""
        cost = self._cost(cost)
        return self._search_rows(self.ctx.lib.wa_grid_weighted_matrix, (_ptr(cost),), ids, True)

    @staticmethod
    def _step(step):
        step = np.ascontiguousarray(step, np.int32).reshape(-1)
        assert step.size == 3, "step holds the costs of a face, an edge and a corner move"
        return step

    def chamfer_fields(self, step, ids):
        """wa_grid_chamfer_fields: int32 [len(ids), n], the exact least sum of step costs on the 26-neighbour lattice of free voxels
        (step = (face, edge, corner), each 1 .. WA_STEP_MAX; a diagonal move needs every voxel of the box it spans free) from each source
        to every voxel; WA_DIST_NONE (-1) where there is no path"""
        step = self._step(step)
        return self._search_rows(self.ctx.lib.wa_grid_chamfer_fields, (_ptr(step),), ids, False)

    def chamfer_matrix(self, step, ids):
        """wa_grid_chamfer_matrix: int32 [P, P] of those distances between the points (symmetric, 0 on the diagonal, WA_DIST_NONE (-1)
        where two points are not connected)"""
        step = self._step(step)
        return self._search_rows(self.ctx.lib.wa_grid_chamfer_matrix, (_ptr(step),), ids, True)

    def _pen(self, pen):
        pen = np.ascontiguousarray(pen, np.uint8).reshape(-1)
        assert pen.size == self.n, "a penalty array holds one byte per voxel"
        return pen

    def chamfer_weighted_fields(self, step, pen, ids):
        """wa_grid_chamfer_weighted_fields: int32 [len(ids), n], the exact least sum of step[class - 1] + pen[voxel entered] over the moves
        of chamfer_fields' graph (pen: uint8 [n], 0 .. WA_PEN_MAX on free voxels; the start is not paid for) from each source to every
        voxel; WA_DIST_NONE (-1) where there is no path"""
        step, pen = self._step(step), self._pen(pen)
        return self._search_rows(self.ctx.lib.wa_grid_chamfer_weighted_fields, (_ptr(step), _ptr(pen)), ids, False)

    def chamfer_weighted_matrix(self, step, pen, ids):
        """wa_grid_chamfer_weighted_matrix: int32 [P, P], [i, j] = dist(point i, point j) (not symmetric: [i, j] - [j, i] = pen[j] -
        pen[i]); WA_DIST_NONE (-1) where two points are not connected"""
        step, pen = self._step(step), self._pen(pen)
        return self._search_rows(self.ctx.lib.wa_grid_chamfer_weighted_matrix, (_ptr(step), _ptr(pen)), ids, True)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.wa_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def shortcut_paths(grid, paths, max_span=128):
    """wa_grid_path_shortcut of a batch of paths (node-id arrays) in one call: ([waypoint node ids per path], float64 lengths)"""
    paths = [np.ascontiguousarray(p, np.int64).reshape(-1) for p in paths]
    ids = np.concatenate(paths) if paths else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    wp = np.empty(max(len(ids), 1), np.int64)
    cnt = np.empty(max(len(paths), 1), np.int32)
    lengths = np.empty(len(paths), np.float64)
    ctx = grid.ctx
    ctx.check(ctx.lib.wa_grid_path_shortcut(grid.h, _ptr(ids), _ptr(off), len(paths), int(max_span), _ptr(wp), _ptr(cnt),
                                       _ptr(lengths) if len(paths) else None))
    return [p[wp[off[k]:off[k] + cnt[k]]] for k, p in enumerate(paths)], lengths


def pose_shortcut_paths(grid, dirs, tool, max_turn, paths, ks, max_span=128):
    """wa_grid_pose_shortcut of a batch of (voxel, direction) paths in one call -- `paths` node-id arrays, `ks` one direction index per
    node, as Grid.pose_paths returns them.  A stretch of a path is replaced by a straight segment only where the two directions are
    within `max_turn` of each other and one of them is open in every voxel the segment touches.  Returns ([waypoint node ids per path],
    [direction index of the path at each waypoint], [hold per segment: the direction that is open along it, -1 for a hop that is not
    held; one entry fewer than waypoints], float64 lengths, summary dict)."""
    dirs, K, tool = grid._torch_args(dirs, tool)
    paths = [np.ascontiguousarray(p, np.int64).reshape(-1) for p in paths]
    ks = [np.ascontiguousarray(k, np.int32).reshape(-1) for k in ks]
    assert len(paths) == len(ks) and all(len(p) == len(k) for p, k in zip(paths, ks)), "one direction index per node"
    ids = np.concatenate(paths) if paths else np.zeros(0, np.int64)
    kk = np.concatenate(ks) if ks else np.zeros(0, np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    wp = np.empty(max(len(ids), 1), np.int64)
    hold = np.empty(max(len(ids), 1), np.int32)
    cnt = np.empty(max(len(paths), 1), np.int32)
    lengths = np.empty(len(paths), np.float64)
    s = L.PoseShortcutSummary()
    pad = np.zeros(1, np.int64)
    ctx = grid.ctx
    ctx.check(ctx.lib.wa_grid_pose_shortcut(grid.h, _ptr(dirs), K, C.byref(tool), int(max_turn), _ptr(ids if len(ids) else pad),
                                            _ptr(kk if len(kk) else np.zeros(1, np.int32)), _ptr(off), len(paths), int(max_span), _ptr(wp),
                                            _ptr(hold), _ptr(cnt), _ptr(lengths) if len(paths) else None, C.byref(s)))
    idx = [wp[off[k]:off[k] + cnt[k]] for k in range(len(paths))]
    return ([p[i] for p, i in zip(paths, idx)], [k[i] for k, i in zip(ks, idx)],
            [hold[off[k]:off[k] + max(cnt[k] - 1, 0)].copy() for k in range(len(paths))], lengths,
            {k: int(getattr(s, k)) for k, _ in L.PoseShortcutSummary._fields_})


def _paths_two_calls(grid, fn, lead, starts, ends, n_counts, lengths):
    """The protocol of the _paths calls, fn(grid, *lead, starts, ends, n, off, ids, *counts) with n_counts int32 arrays of per-pair counts
    (the first is negative where there is no path): the first call, with empty ranges, returns the counts (WA_ERR_CAPACITY is its
    expected status when any pair is reachable); lengths(*counts) then sizes the ranges and the second call writes the paths into them.
    Returns (counts, [node-id array per pair, start first; None where there is no path])."""
    starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
    ends = np.ascontiguousarray(ends, np.int64).reshape(-1)
    assert len(starts) == len(ends)
    n = len(starts)
    ctx = grid.ctx
    counts = [np.zeros(max(n, 1), np.int32) for _ in range(n_counts)]
    off = np.zeros(n + 1, np.int64)
    pad = np.zeros(1, np.int64)
    rc = fn(grid.h, *lead, _ptr(starts if n else pad), _ptr(ends if n else pad), n, _ptr(off), _ptr(pad), *[_ptr(c) for c in counts])
    if rc not in (0, 7):
        ctx.check(rc)
    off[1:] = np.cumsum(lengths(*[c[:n].astype(np.int64) for c in counts]))
    ids = np.empty(max(int(off[-1]), 1), np.int64)
    if rc == 7:
        ctx.check(fn(grid.h, *lead, _ptr(starts), _ptr(ends), n, _ptr(off), _ptr(ids), *[_ptr(c) for c in counts]))
    counts = [c[:n] for c in counts]
    return counts, [ids[off[k]:off[k + 1]].copy() if counts[0][k] >= 0 else None for k in range(n)]


def geodesic_paths(grid, starts, ends):
    """wa_grid_geodesic_paths of a batch of pairs: (int32 hops, [node-id array per pair, start first; None where hops is WA_HOPS_NONE]),
    the paths in ranges of hops + 1 ids (_paths_two_calls)"""
    (hops,), paths = _paths_two_calls(grid, grid.ctx.lib.wa_grid_geodesic_paths, (), starts, ends, 1, lambda hops: np.maximum(hops + 1, 0))
    return hops, paths


def weighted_paths(grid, cost, starts, ends):
    """wa_grid_weighted_paths of a batch of pairs: (int32 dist, int32 node counts, [node-id array per pair, start first; None where dist
    is WA_DIST_NONE]), the paths in ranges of len ids (_paths_two_calls)"""
    cost = grid._cost(cost)
    (dist, lens), paths = _paths_two_calls(grid, grid.ctx.lib.wa_grid_weighted_paths, (_ptr(cost),), starts, ends, 2, lambda dist, lens: lens)
    return dist, lens, paths


def chamfer_paths(grid, step, starts, ends):
    """wa_grid_chamfer_paths of a batch of pairs: (int32 dist, int32 node counts, [node-id array per pair, start first; None where dist
    is WA_DIST_NONE]), the paths in ranges of len ids (_paths_two_calls)"""
    step = grid._step(step)
    (dist, lens), paths = _paths_two_calls(grid, grid.ctx.lib.wa_grid_chamfer_paths, (_ptr(step),), starts, ends, 2, lambda dist, lens: lens)
    return dist, lens, paths


def chamfer_weighted_paths(grid, step, pen, starts, ends):
    """wa_grid_chamfer_weighted_paths of a batch of pairs: (int32 dist, int32 node counts, [node-id array per pair, start first; None
    where dist is WA_DIST_NONE]), the paths in ranges of len ids (_paths_two_calls)"""
    step, pen = grid._step(step), grid._pen(pen)
    (dist, lens), paths = _paths_two_calls(grid, grid.ctx.lib.wa_grid_chamfer_weighted_paths, (_ptr(step), _ptr(pen)), starts, ends, 2,
                                           lambda dist, lens: lens)
    return dist, lens, paths


def default_params(**kw):
    p = AcsParams()
    L.load().wa_acs_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class AcsSolver:
    def __init__(self, ctx, grid, n_slots=1, max_colony=256, path_capacity=0, neighbourhood=6, lazy=False):
        self.ctx, self.grid, self.n_slots, self.max_colony, self.nb = ctx, grid, n_slots, max_colony, neighbourhood
        h = C.c_void_p()
        if lazy:
            ctx.check(ctx.lib.wa_acs_create_lazy_nb(ctx.h, grid.h, n_slots, max_colony, path_capacity, neighbourhood, C.byref(h)))
        else:
            ctx.check(ctx.lib.wa_acs_create_nb(ctx.h, grid.h, n_slots, max_colony, path_capacity, neighbourhood, C.byref(h)))
        self.h = h
        self.iters = 0
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.wa_acs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def init_pheromone(self, p0=1.0, slot=-1):
        self.ctx.check(self.ctx.lib.wa_acs_init_pheromone(self.h, slot, C.c_float(p0)))

    def reset_pheromone(self, p0=1.0, slot=-1):
        self.ctx.check(self.ctx.lib.wa_acs_reset_pheromone(self.h, slot, C.c_float(p0)))

    def srand(self, seed):
        self.ctx.check(self.ctx.lib.wa_acs_srand(self.h, seed & 0xFFFFFFFF))

    def rand_state(self, state=None):
        st = np.zeros(36, np.int32) if state is None else np.ascontiguousarray(state, np.int32)
        self.ctx.check(self.ctx.lib.wa_acs_rand_state(self.h, _ptr(st), 0 if state is None else 1))
        return st

    def _arrs(self, starts, ends, streams):
        starts = np.ascontiguousarray(np.atleast_1d(starts), np.int64)
        ends = np.ascontiguousarray(np.atleast_1d(ends), np.int64)
        streams = None if streams is None else np.ascontiguousarray(np.atleast_1d(streams), np.uint32)
        return starts, ends, streams

    def begin(self, params, starts, ends, streams=None):
        starts, ends, streams = self._arrs(starts, ends, streams)
        self.n_active = len(starts)
        self.iters = params.max_iteration
        self.ctx.check(self.ctx.lib.wa_acs_begin(self.h, C.byref(params), len(starts), _ptr(starts), _ptr(ends), _ptr(streams)))

    def run(self, n_generations):
        self.ctx.check(self.ctx.lib.wa_acs_run(self.h, n_generations))

    def sync(self):
        self.ctx.check(self.ctx.lib.wa_acs_sync(self.h))

    def straggler_counters(self, slot=0, reset=False):
        """(ants handed over, stragglers finished by a resume block) of one slot"""
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.wa_acs_straggler_counters(self.h, slot, C.byref(a), C.byref(b), 1 if reset else 0))
        return a.value, b.value

    def converged_info(self, slot=0):
        """converged generations in one launch, for one slot since the solver was created: windows enqueued, committed whole, cut short by an
        ant that left the best path, and generations committed"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.ctx.lib.wa_acs_converged_info(self.h, slot, out))
        return dict(enqueued=int(out[0]), whole=int(out[1]), cut=int(out[2]), generations=int(out[3]))

    def converged_host_info(self):
        """what run() did with the windows' verdicts since the solver was created (a lone search): verdicts it went to read, generations whose
        launches it did not enqueue, speculative launches cancelled, waits given up"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.ctx.lib.wa_acs_converged_host_info(self.h, out))
        return [int(v) for v in out]

    def converged_owed_info(self):
        """owed evaporations (a lone search whose verdicts run() reads) since the solver was created: whole windows found carried, generations
        enqueued whose sweep paid a carried window's evaporations with its own (`merged`), whole windows that were not carried and flushed as ever
        (`fallback`), and of the merged sweeps those that ran out of place and in place"""
        out = (C.c_uint64 * 5)()
        self.ctx.check(self.ctx.lib.wa_acs_converged_owed_info(self.h, out))
        return dict(carried=int(out[0]), merged=int(out[1]), fallback=int(out[2]), out_of_place=int(out[3]), in_place=int(out[4]))

    def converged_carried_info(self):
        """the carried walk (where owed evaporations apply) since the solver was created: walk launches that took the carried path, rows launches
        of carried windows that were not enqueued, walk launches enqueued ahead of their window's verdict and, of those, the cancelled ones"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.ctx.lib.wa_acs_converged_carried_info(self.h, out))
        return dict(walks=int(out[0]), rows_skipped=int(out[1]), spec_walks=int(out[2]), spec_cancelled=int(out[3]))

    def set_stragglers(self, generations):
        """generations of a search during which ants may be handed over (0: off, < 0: default)"""
        self.ctx.check(self.ctx.lib.wa_acs_set_stragglers(self.h, generations))

    def set_pipeline(self, groups):
        """groups of slots that advance on streams of their own inside run() (0: by rule, 1: one stream)"""
        self.ctx.check(self.ctx.lib.wa_acs_set_pipeline(self.h, groups))

    def pipeline_groups(self):
        g = C.c_int32()
        self.ctx.check(self.ctx.lib.wa_acs_pipeline_info(self.h, C.byref(g)))
        return g.value

    def solve(self, params, starts, ends, streams=None):
        starts, ends, streams = self._arrs(starts, ends, streams)
        self.n_active = len(starts)
        self.iters = params.max_iteration
        self.ctx.check(self.ctx.lib.wa_acs_solve(self.h, C.byref(params), len(starts), _ptr(starts), _ptr(ends), _ptr(streams)))

    def result(self, slot=0):
        cost, n = C.c_float(), C.c_int64()
        self.ctx.check(self.ctx.lib.wa_acs_result(self.h, slot, C.byref(cost), C.byref(n), None, None, 0))
        ids = np.empty(n.value, np.int32)
        ch = np.empty(max(n.value - 1, 0), np.int8)
        if n.value:
            self.ctx.check(self.ctx.lib.wa_acs_result(self.h, slot, C.byref(cost), C.byref(n), _ptr(ids), _ptr(ch), n.value))
        return np.float32(cost.value), ids, ch

    def results(self, n_slots=None):
        """(costs, [path ids per slot]) of slots 0..n_slots-1 in one round trip"""
        n = self.n_slots if n_slots is None else n_slots
        costs, lens = np.empty(n, np.float32), np.empty(n, np.int64)
        self.ctx.check(self.ctx.lib.wa_acs_result_batch(self.h, n, _ptr(costs), _ptr(lens), None, 0))
        stride = int(lens.max()) if n else 0
        buf = np.empty((n, max(stride, 1)), np.int32)
        if stride:
            self.ctx.check(self.ctx.lib.wa_acs_result_batch(self.h, n, _ptr(costs), _ptr(lens), _ptr(buf), stride))
        return costs, [buf[q, :lens[q]].copy() for q in range(n)]

    def trace(self, slot=0):
        g = C.c_int32()
        self.ctx.check(self.ctx.lib.wa_acs_trace(self.h, slot, C.byref(g), None, None, None, None, None))
        n = g.value
        t = dict(bestL=np.zeros(n, np.float32), iterbestL=np.zeros(n, np.float32), colony=np.zeros(n, np.int32),
                 finite=np.zeros(n, np.int32), steps=np.zeros(n, np.int64))
        self.ctx.check(self.ctx.lib.wa_acs_trace(self.h, slot, C.byref(g), _ptr(t["bestL"]), _ptr(t["iterbestL"]),
                                                 _ptr(t["colony"]), _ptr(t["finite"]), _ptr(t["steps"])))
        return t

    def export_trace(self, dst_device_ptr, gen0, count):
        self.ctx.check(self.ctx.lib.wa_acs_export_trace(self.h, dst_device_ptr, gen0, count))

    def pheromone(self, slot=0):
        out = np.empty(self.grid.n * self.nb, np.float32)
        self.ctx.check(self.ctx.lib.wa_acs_read_pheromone(self.h, slot, _ptr(out)))
        return out

    def ants(self, slot=0):
        """(L, node count) per ant of the generation walked last"""
        c = C.c_int32()
        self.ctx.check(self.ctx.lib.wa_acs_read_ants(self.h, slot, C.byref(c), None, None, 0))
        Ls, lens = np.empty(c.value, np.float32), np.empty(c.value, np.int32)
        self.ctx.check(self.ctx.lib.wa_acs_read_ants(self.h, slot, C.byref(c), _ptr(Ls), _ptr(lens), c.value))
        return Ls, lens

    def ant_path(self, ant, slot=0):
        """node ids visited by one ant of the generation walked last (Agent::getPath())"""
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.wa_acs_read_ant_path(self.h, slot, ant, None, 0, C.byref(n)))
        ids = np.empty(n.value, np.int32)
        self.ctx.check(self.ctx.lib.wa_acs_read_ant_path(self.h, slot, ant, _ptr(ids), n.value, C.byref(n)))
        return ids

    def last_params(self, slot=0):
        c, l, q = C.c_int32(), C.c_float(), C.c_float()
        self.ctx.check(self.ctx.lib.wa_acs_last_params(self.h, slot, C.byref(c), C.byref(l), C.byref(q)))
        return c.value, np.float32(l.value), np.float32(q.value)

    def walk_info(self):
        """what the last DEV walk launch ran with (wa_acs_walk_info): table size, 16-bit entries or not, LDS per walk block, resident blocks per CU"""
        v = (C.c_int32 * 4)()
        self.ctx.check(self.ctx.lib.wa_acs_walk_info(self.h, v))
        lds = int(v[2])
        return dict(hash_log2=int(v[0]), entries16=bool(v[1]), lds_bytes_per_block=lds, resident_blocks_per_cu=min(163840 // lds, 16) if lds else 0, touch_loads=bool(v[3]))

    def profile(self, enable=True, sample_every=1, sweep_every_generation=False, paired=False):
        """paired: every timed sweep-carrying launch is preceded by a stamped no-op dispatch (wa_acs_profile bit 2; why: profiles/r06/sweep_gap.txt)"""
        self.ctx.check(self.ctx.lib.wa_acs_profile(self.h, ((3 if sweep_every_generation else 1) | (4 if paired else 0)) if enable else 0, sample_every))

    def profile_read(self):
        ms = np.zeros(L.K_COUNT, np.float64)
        n = np.zeros(L.K_COUNT, np.int64)
        self.ctx.check(self.ctx.lib.wa_acs_profile_read(self.h, _ptr(ms), _ptr(n)))
        names = ["walk", "rank", "evaporate", "deposit"]
        return {k: dict(ms=float(ms[i]), launches=int(n[i])) for i, k in enumerate(names)}

    def evaporate(self, slot=0, rho=0.8, repeats=1):
        self.ctx.check(self.ctx.lib.wa_acs_evaporate(self.h, slot, C.c_float(rho), repeats))


def memory_estimate(grid, max_colony, path_capacity=0, neighbourhood=6, lazy=False):
    """(bytes per slot, bytes per heuristic field, fixed bytes) of a solver of this shape (wa_acs_memory_estimate)"""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    grid.ctx.check(grid.ctx.lib.wa_acs_memory_estimate(grid.h, max_colony, path_capacity, neighbourhood, 1 if lazy else 0,
                                                       C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def straggler_pool_bytes(grid, n_slots, max_colony, path_capacity=0, neighbourhood=6, lazy=False):
    """bytes of arrival lists + straggler pools a solver of this shape holds (0 when it gets none)"""
    b = C.c_int64()
    grid.ctx.check(grid.ctx.lib.wa_acs_straggler_pool_bytes(grid.h, n_slots, max_colony, path_capacity, neighbourhood, 1 if lazy else 0, C.byref(b)))
    return b.value


def pack_best_key(cost, rank, slot, lib_path=None):
    """the 64-bit key of the global-best exchange (host-side helper of the library: cost bits << 32 | rank << 16 | slot)"""
    k = C.c_uint64()
    rc = L.load(lib_path).wa_comm_pack_best_key(C.c_float(cost), rank, slot, C.byref(k))
    if rc:
        raise WeldacsError(rc, "wa_comm_pack_best_key")
    return k.value


def unpack_best_key(key, lib_path=None):
    c, r, s_ = C.c_float(), C.c_int32(), C.c_int32()
    L.load(lib_path).wa_comm_unpack_best_key(C.c_uint64(int(key)), C.byref(c), C.byref(r), C.byref(s_))
    return np.float32(c.value), r.value, s_.value


def pair_slots_by_rule(ctx, grid, colony, n_pairs, n_ends, max_iteration, lazy=True, neighbourhood=6, all_fields=False):
    """Concurrent pair searches for `n_pairs` searches on this device -- the rule of the drop-in ACS_Rank::slots_for
    (welding_robot_amd/include/core/ACSRank_3D.hpp): 3/4 of the free memory but at most ~200 GB of fields, at most three
    rounds of resident walk blocks, then whole batches of equal size.  Returns (slots, batches)."""
    per_slot, per_field, fixed = memory_estimate(grid, colony, 0, neighbourhood, lazy)
    per_slot += 20 * max_iteration
    free, _ = ctx.memory_info()
    fields = max(4, n_ends) if all_fields else min(max(4, n_ends), 8)   # (all_fields: every end point's heuristic field stays resident)
    cap = (min(free // 4 * 3, int(200e9)) - fixed - fields * per_field) // per_slot
    cap = max(1, min(cap, max(1, 3 * 2048 // colony)))
    batches = -(-n_pairs // cap)
    return -(-n_pairs // batches), batches


class Comm:
    """wa_comm: RCCL communicator behind the C ABI (csrc/host_comm.inc) -- the global-best exchange of the multi-GPU path.
    Rank 0 makes the id (Comm.unique_id()), the caller ships the 128 bytes to the other ranks."""

    @staticmethod
    def unique_id(lib_path=None):
        buf = np.zeros(128, np.uint8)
        rc = L.load(lib_path).wa_comm_unique_id(_ptr(buf))
        if rc:
            raise WeldacsError(rc, "wa_comm_unique_id failed")
        return buf

    def __init__(self, ctx, rank, world, uid):
        self.ctx = ctx
        uid = np.ascontiguousarray(uid, np.uint8)
        assert uid.size == 128
        h = C.c_void_p()
        ctx.check(ctx.lib.wa_comm_create(ctx.h, rank, world, _ptr(uid), C.byref(h)))
        self.h, self.rank, self.world = h, rank, world
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.wa_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def abort(self):
        """give the communicator up now (wa_comm_abort -> ncclCommAbort): every later call fails with WA_ERR_STATE"""
        self.ctx.check(self.ctx.lib.wa_comm_abort(self.h))

    def stats(self):
        """what RCCL itself says about this communicator, and what was issued on it (wa_comm_stats)"""
        v = (C.c_int64 * 5)()
        self.ctx.check(self.ctx.lib.wa_comm_stats(self.h, v))
        return dict(ranks=int(v[0]), version=int(v[1]), allreduce_calls=int(v[2]), other_calls=int(v[3]), aborted=bool(v[4]))

    def allreduce_best(self, solver, gen0, count):
        """asynchronous: MIN over ranks (and active slots) of best_L[gen0 .. gen0+count)"""
        self.ctx.check(self.ctx.lib.wa_acs_allreduce_best(solver.h, self.h, gen0, count))

    def read_best(self, gen0, count):
        out = np.empty(count, np.float32)
        self.ctx.check(self.ctx.lib.wa_comm_read_best(self.h, gen0, count, _ptr(out)))
        return out

    def read_best_owner(self, gen0, count):
        """(global best cost, owner rank, owner slot) per generation: whose search holds the path that achieved it"""
        cost, rk, sl = np.empty(count, np.float32), np.empty(count, np.int32), np.empty(count, np.int32)
        self.ctx.check(self.ctx.lib.wa_comm_read_best_owner(self.h, gen0, count, _ptr(cost), _ptr(rk), _ptr(sl)))
        return cost, rk, sl

    def allgather_costs(self, index, cost, n_total, fill=np.nan):
        """every rank's (pair index, cost) records to every rank: a vector of n_total costs (entries nobody owns = fill)"""
        index = np.ascontiguousarray(index, np.int32)
        cost = np.ascontiguousarray(cost, np.float32)
        assert index.shape == cost.shape
        out = np.full(n_total, fill, np.float32)
        self.ctx.check(self.ctx.lib.wa_comm_allgather_costs(self.h, index.size, _ptr(index), _ptr(cost), n_total, _ptr(out)))
        return out

    def gather_paths(self, paths, root=0):
        """paths: {global index: node ids} of this rank.  On `root`: {index: ids} of ALL ranks; elsewhere {}."""
        keys = list(paths)
        index = np.ascontiguousarray(keys, np.int32)
        lens = np.ascontiguousarray([len(paths[k]) for k in keys], np.int64)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(paths[k], np.int32) for k in keys]) if keys else np.zeros(0), np.int32)
        npaths, nids = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.wa_comm_gather_paths(self.h, root, index.size, _ptr(index), _ptr(lens), _ptr(ids), C.byref(npaths), C.byref(nids)))
        if self.rank != root:
            return {}
        self.ctx.check(self.ctx.lib.wa_comm_gathered_paths_counts(self.h, C.byref(npaths), C.byref(nids)))   # what the read below copies out
        gi, gl, gd = np.empty(npaths.value, np.int32), np.empty(npaths.value, np.int64), np.empty(nids.value, np.int32)
        self.ctx.check(self.ctx.lib.wa_comm_gathered_paths_read(self.h, _ptr(gi), _ptr(gl), _ptr(gd)))
        off = np.concatenate([[0], np.cumsum(gl)])
        return {int(gi[i]): gd[off[i]:off[i + 1]].copy() for i in range(npaths.value)}

    def broadcast_grid(self, grid, root=0):
        """wa_comm_broadcast_grid: rank `root` passes its Grid, every other rank None; everybody gets a Grid back (the root its own)"""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.wa_comm_broadcast_grid(self.h, root, grid.h if grid is not None else None, C.byref(h)))
        if self.rank == root:
            return grid
        return Grid(self.ctx, h)

    def allreduce(self, values, op="max"):
        v = np.ascontiguousarray(np.atleast_1d(values), np.float64).copy()
        self.ctx.check(self.ctx.lib.wa_comm_allreduce_f64(self.h, _ptr(v), v.size, {"min": 0, "max": 1, "sum": 2}[op]))
        return v

    def barrier(self):
        self.ctx.check(self.ctx.lib.wa_comm_barrier(self.h))


class Trajectory:
    """Device-resident polyline (n x 3 floats): a stitched path or a sampled spline."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        ctx._children.add(self)

    @classmethod
    def from_points(cls, ctx, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        h = C.c_void_p()
        ctx.check(ctx.lib.wa_traj_from_points(ctx.h, _ptr(xyz), len(xyz), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def stitch(cls, grid, segments, reverse=None):
        """ACS_GTSP::read_all_segments: `segments` = list of node-id arrays in tour order."""
        segs = [np.ascontiguousarray(s, np.int64).reshape(-1) for s in segments]
        ids = np.concatenate(segs) if segs else np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
        rev = np.ascontiguousarray(reverse, np.uint8) if reverse is not None else None
        h = C.c_void_p()
        ctx = grid.ctx
        ctx.check(ctx.lib.wa_traj_stitch(grid.h, _ptr(ids), _ptr(off), len(segs), _ptr(rev), C.byref(h)))
        return cls(ctx, h)

    def __len__(self):
        return int(self.ctx.lib.wa_traj_size(self.h))

    def points(self):
        out = np.empty((len(self), 3), np.float32)
        self.ctx.check(self.ctx.lib.wa_traj_read(self.h, _ptr(out)))
        return out

    def clearance(self, grid):
        """wa_traj_clearance: (voxel ids int64[n], d2 int32[n], hits uint8[n-1], summary dict)"""
        n = len(self)
        ids, d2, hit = np.empty(n, np.int64), np.empty(n, np.int32), np.empty(max(n - 1, 0), np.uint8)
        s = L.ClearanceSummary()
        self.ctx.check(self.ctx.lib.wa_traj_clearance(grid.h, self.h, _ptr(ids), _ptr(d2), _ptr(hit) if len(hit) else None, C.byref(s)))
        summary = {k: int(getattr(s, k)) for k, _ in L.ClearanceSummary._fields_}
        return ids, d2, hit, summary

    def fit(self, grid, degree=3, spacing=None, max_level=6, n_samples=6001):
        """wa_grid_fit_trajectory with this polyline: control points on the polyline, refined leg by leg until the sampled curve clears
        `grid` (the metal).  spacing=None: one voxel (grid.precision).  Returns (Bspline, samples Trajectory, levels int32[n-1], summary dict;
        summary["final"] is the clearance summary of the samples)."""
        spacing = grid.precision if spacing is None else spacing
        levels = np.empty(max(len(self) - 1, 0), np.int32)
        bh, th, s = C.c_void_p(), C.c_void_p(), L.FitSummary()
        self.ctx.check(self.ctx.lib.wa_grid_fit_trajectory(grid.h, self.h, degree, C.c_float(spacing), max_level, n_samples, _ptr(levels),
                                                           C.byref(bh), C.byref(th), C.byref(s)))
        summary = {k: int(getattr(s, k)) for k, _ in L.FitSummary._fields_ if k != "final"}
        summary["final"] = {k: int(getattr(s.final, k)) for k, _ in L.ClearanceSummary._fields_}
        return Bspline.adopt(self.ctx, bh, 3, degree, summary["n_cps"] - 2 * degree), Trajectory(self.ctx, th), levels, summary

    def pose_fit(self, grid, dirs, tool, holds, degree=3, spacing=None, max_level=6, n_samples=6001):
        """wa_grid_pose_fit_trajectory with this polyline: the loop of fit(), refined until one of the planned directions -- `holds`, one
        per leg, -1 for none, as pose_shortcut_paths returns them -- is open for `tool` in every voxel each piece of the sampled curve
        touches.  Returns (Bspline, samples Trajectory, levels int32[n-1], seg_dir int32[n_samples-1]: the direction found for every
        segment, -1 for none, blocked uint8[n_samples-1], summary dict; summary["final"] is the occupancy clearance summary of the
        samples, summary["n_blocked"] == 0 the success case)."""
        spacing = grid.precision if spacing is None else spacing
        dirs, K, tool = grid._torch_args(dirs, tool)
        holds = np.ascontiguousarray(holds, np.int32).reshape(-1)
        if len(holds) != len(self) - 1:
            raise ValueError("holds needs one entry per leg")
        levels = np.empty(max(len(self) - 1, 0), np.int32)
        seg_dir, blocked = np.empty(max(n_samples - 1, 0), np.int32), np.empty(max(n_samples - 1, 0), np.uint8)
        bh, th, s = C.c_void_p(), C.c_void_p(), L.PoseFitSummary()
        self.ctx.check(self.ctx.lib.wa_grid_pose_fit_trajectory(grid.h, self.h, degree, C.c_float(spacing), max_level, n_samples, _ptr(dirs), K,
                                                                C.byref(tool), _ptr(holds), _ptr(levels), C.byref(bh), C.byref(th),
                                                                _ptr(seg_dir), _ptr(blocked), C.byref(s)))
        summary = {k: int(getattr(s, k)) for k, _ in L.PoseFitSummary._fields_ if k != "final"}
        summary["final"] = {k: int(getattr(s.final, k)) for k, _ in L.ClearanceSummary._fields_}
        return (Bspline.adopt(self.ctx, bh, 3, degree, summary["n_cps"] - 2 * degree), Trajectory(self.ctx, th), levels, seg_dir, blocked,
                summary)

    def retime(self, v_max, acc, dec, tick, a_lat=float("inf"), grid=None, v_near=0.0, near_d2=-1, v_limit=None, ticks=True):
        """wa_traj_retime with these samples: the fastest rest-to-rest speed profile under the caps (v_max, the per-sample v_limit, a_lat
        over the curvature, v_near where `grid`'s distance field is <= near_d2) and the ramps acc / dec, and the positions every `tick`
        seconds.  Returns (time_q int64[n], w_q int64[n], bound uint8[n], ticks Trajectory or None, summary dict); times and squared
        speeds are in quanta of 2^-30 (RETIME_Q)."""
        n = len(self)
        lim = L.RetimeLimits(v_max, acc, dec, a_lat, v_near, near_d2)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        time_q, w_q, bound = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
        th, s = C.c_void_p(), L.RetimeSummary()
        rc = self.ctx.lib.wa_traj_retime(grid.h if grid is not None else None, self.h, C.byref(lim), _ptr(v_limit), C.c_double(tick),
                                         _ptr(time_q), _ptr(w_q), _ptr(bound), C.byref(th) if ticks else None, C.byref(s))
        if rc != 7:   # WA_ERR_CAPACITY: everything but the ticks is there
            self.ctx.check(rc)
        summary = {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in L.RetimeSummary._fields_}
        return time_q, w_q, bound, Trajectory(self.ctx, th) if th.value else None, summary

    def torch_axes(self, grid, dirs, tool, w_near=1, w_want=0, w_turn=1, near_add=-1, max_turn=-1, want=None, off=None, pin_first=None,
                   pin_last=None, feas=True):
        """wa_traj_tool_axes with these samples as the torch tip: for every sample one of the K directions `dirs` (K x 3, tip -> body) so
        that the beads of `tool` (torch_tool(dist16, r2), or that pair) stay clear of `grid`'s metal and the direction turns little.
        `off`: n_legs + 1 offsets of independent legs (None: one leg); want: n x 3 wished directions (zero rows: none).  Returns
        dict(dir int32[n], feas uint8[n, K] (255 = blocked, else the near beads; None with feas=False), leg_cost int64[n_legs], summary)."""
        n = len(self)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        K = len(dirs)
        tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        w = L.ToolWeights(w_near, w_want, w_turn, near_add, max_turn)
        off = np.ascontiguousarray([0, n] if off is None else off, np.int64).reshape(-1)
        n_legs = len(off) - 1
        if want is not None:
            want = np.ascontiguousarray(want, np.float32).reshape(-1, 3)
            if len(want) != n:
                raise ValueError("want needs one row per sample")
        pins = []
        for p in (pin_first, pin_last):
            p = None if p is None else np.ascontiguousarray(p, np.int32).reshape(-1)
            if p is not None and len(p) != n_legs:
                raise ValueError("pins need one entry per leg")
            pins.append(p)
        dir_out, leg_cost = np.empty(n, np.int32), np.empty(max(n_legs, 0), np.int64)
        feas_out = np.empty((n, K), np.uint8) if feas else None
        s = L.ToolSummary()
        self.ctx.check(self.ctx.lib.wa_traj_tool_axes(grid.h, self.h, _ptr(dirs), K, C.byref(tool), C.byref(w), _ptr(want), _ptr(off), n_legs,
                                                      _ptr(pins[0]), _ptr(pins[1]), _ptr(dir_out), _ptr(feas_out), _ptr(leg_cost), C.byref(s)))
        return dict(dir=dir_out, feas=feas_out, leg_cost=leg_cost, summary={k: int(getattr(s, k)) for k, _ in L.ToolSummary._fields_})

    def torch_check(self, grid, axes, tool, near_add=-1):
        """wa_traj_tool_check: one given axis per sample (n x 3) against the same bead rule; (blocked uint8[n], near uint8[n], summary)"""
        n = len(self)
        axes = np.ascontiguousarray(axes, np.float32).reshape(-1, 3)
        if len(axes) != n:
            raise ValueError("axes needs one row per sample")
        tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        blocked, near = np.empty(n, np.uint8), np.empty(n, np.uint8)
        s = L.ToolSummary()
        self.ctx.check(self.ctx.lib.wa_traj_tool_check(grid.h, self.h, _ptr(axes), C.byref(tool), near_add, _ptr(blocked), _ptr(near), C.byref(s)))
        return blocked, near, {k: int(getattr(s, k)) for k, _ in L.ToolSummary._fields_}

    def _axes(self, q):
        q = np.ascontiguousarray(q, np.int32).reshape(-1, 3)
        if len(q) != len(self):
            raise ValueError("q needs one quantised axis (quantise_axes) per sample")
        return q

    def smooth_axes(self, q, h, max_level=8, grid=None, tool=None, off=None):
        """wa_traj_axes_smooth: the quantised axes `q` (int32 n x 3, quantise_axes) averaged over windows of half-width `h` along the path,
        per sample the widest window (h, h/2, ... down to the sample's own axis at level max_level) whose average keeps the beads of
        `tool` clear of `grid`'s metal; `off` splits the samples into legs that no window crosses.  grid and tool come together or not
        at all.  Returns dict(q int32[n, 3], level uint8[n], blocked uint8[n], summary)."""
        n = len(self)
        q = self._axes(q)
        if tool is not None:
            tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        off = np.ascontiguousarray([0, n] if off is None else off, np.int64).reshape(-1)
        q_out, level, blocked = np.empty((n, 3), np.int32), np.empty(n, np.uint8), np.empty(n, np.uint8)
        s = L.AxesSmoothSummary()
        self.ctx.check(self.ctx.lib.wa_traj_axes_smooth(grid.h if grid is not None else None, self.h, _ptr(q), C.byref(tool) if tool is not None else None,
                                                        _ptr(off), len(off) - 1, C.c_double(h), max_level, _ptr(q_out), _ptr(level), _ptr(blocked),
                                                        C.byref(s)))
        summary = {k: (list(getattr(s, k)) if k == "n_level" else int(getattr(s, k))) for k, _ in L.AxesSmoothSummary._fields_}
        return dict(q=q_out, level=level, blocked=blocked, summary=summary)

    def axis_limits(self, q, omega, v_cap, v_floor, v_limit=None):
        """wa_traj_axes_limits: the per-sample speed limit under which the axes `q` turn at no more than `omega` (chord of the unit axes
        per second), capped at v_cap, combined with `v_limit` and raised to v_floor where it falls below.  Returns (float32[n] for
        retime(v_limit=...), summary)."""
        n = len(self)
        q = self._axes(q)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        out = np.empty(n, np.float32)
        s = L.AxesLimitsSummary()
        self.ctx.check(self.ctx.lib.wa_traj_axes_limits(self.h, _ptr(q), C.c_double(omega), C.c_double(v_cap), C.c_double(v_floor), _ptr(v_limit),
                                                        _ptr(out), C.byref(s)))
        return out, {k: (float(s.min_limit) if k == "min_limit" else int(getattr(s, k))) for k, _ in L.AxesLimitsSummary._fields_}

    def tick_axes(self, q, time_q, w_q, acc, dec, tick, grid=None, tool=None, near_add=-1, axes=True, blocked=True):
        """wa_traj_tick_axes: the axis at every controller tick of retime(...)'s result (time_q, w_q, the same acc, dec and tick), the
        sample axes `q` interpolated along each segment like the position, each checked against `grid` with `tool` at the tick's
        position.  Returns (Trajectory of n_ticks unit axes or None, blocked uint8[n_ticks] or None, summary)."""
        n = len(self)
        q = self._axes(q)
        time_q = np.ascontiguousarray(time_q, np.int64).reshape(-1)
        w_q = np.ascontiguousarray(w_q, np.int64).reshape(-1)
        if len(time_q) != n or len(w_q) != n:
            raise ValueError("time_q and w_q need one entry per sample")
        if tool is not None:
            tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        out = None
        if blocked and n >= 2:
            tq = int(np.rint(np.float64(tick) * RETIME_Q)) if np.isfinite(tick) else 0
            n_ticks = int(time_q[-1]) // tq + 1 + (1 if int(time_q[-1]) % tq else 0) if tq >= 1 and time_q[-1] >= 0 else 0
            out = np.empty(n_ticks if n_ticks <= 1 << 31 else 0, np.uint8)
        th, s = C.c_void_p(), L.TickAxesSummary()
        self.ctx.check(self.ctx.lib.wa_traj_tick_axes(grid.h if grid is not None else None, self.h, _ptr(q), C.byref(tool) if tool is not None else None,
                                                      near_add, C.c_double(acc), C.c_double(dec), C.c_double(tick), _ptr(time_q), _ptr(w_q),
                                                      C.byref(th) if axes else None, _ptr(out), C.byref(s)))
        summary = {k: int(getattr(s, k)) for k, _ in L.TickAxesSummary._fields_}
        return Trajectory(self.ctx, th) if th.value else None, out, summary

    def _dwells(self, dwell, what):
        if dwell is None:
            return None
        dwell = np.ascontiguousarray(dwell, np.float64).reshape(-1)
        if len(dwell) != len(self) - 1:
            raise ValueError("%s needs one entry per segment" % what)
        return dwell

    def retime_stops(self, v_max, acc, dec, tick, dwell=None, a_lat=float("inf"), grid=None, v_near=0.0, near_d2=-1, v_limit=None, ticks=True):
        """wa_traj_retime_stops: retime() with stops inside the motion.  dwell: one entry per segment, < 0 for an ordinary segment, >= 0
        for a stop of that many seconds on a segment without length (a doubled sample): the torch comes to rest there, waits and goes on.
        Returns retime()'s tuple and the stops summary: (time_q, w_q, bound, ticks Trajectory or None, summary, stops dict)."""
        n = len(self)
        lim = L.RetimeLimits(v_max, acc, dec, a_lat, v_near, near_d2)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        dwell = self._dwells(dwell, "dwell")
        time_q, w_q, bound = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
        th, s, s2 = C.c_void_p(), L.RetimeSummary(), L.StopsSummary()
        rc = self.ctx.lib.wa_traj_retime_stops(grid.h if grid is not None else None, self.h, C.byref(lim), _ptr(v_limit), _ptr(dwell),
                                               C.c_double(tick), _ptr(time_q), _ptr(w_q), _ptr(bound), C.byref(th) if ticks else None,
                                               C.byref(s), C.byref(s2))
        if rc != 7:   # WA_ERR_CAPACITY: everything but the ticks is there
            self.ctx.check(rc)
        summary = {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in L.RetimeSummary._fields_}
        return time_q, w_q, bound, Trajectory(self.ctx, th) if th.value else None, summary, {k: int(getattr(s2, k)) for k, _ in L.StopsSummary._fields_}

    def retime_jerk(self, v_max, acc, dec, tick, window, dwell=None, seg_tag=None, a_lat=float("inf"), grid=None, v_near=0.0, near_d2=-1,
                    v_limit=None, ticks=True, s_q=False, tags=None):
        """wa_traj_retime_jerk: retime_stops() whose ticks are a moving average of `window` ticks along the arc length (jerk_window()
        sizes it from a jerk limit).  The torch stays on the polyline, the caps are lowered over the window's reach before the profile is
        computed and every dwell keeps its full number of rest ticks.  seg_tag: one byte per segment, carried to the ticks with
        tags=True (the default when seg_tag is given); s_q=True also returns the filtered arc length per tick (quanta of 2^-30).
        Returns (time_q, w_q, bound, ticks Trajectory or None, s_q int64 or None, tags uint8 or None, summary, stops dict, jerk dict);
        the per-sample outputs and `summary` describe the underlying profile.  The host arrays s_q and tags are sized by a first
        call without outputs (the same bytes on every call)."""
        n = len(self)
        lim = L.RetimeLimits(v_max, acc, dec, a_lat, v_near, near_d2)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        dwell = self._dwells(dwell, "dwell")
        if seg_tag is not None:
            seg_tag = np.ascontiguousarray(seg_tag, np.uint8).reshape(-1)
            if len(seg_tag) != n - 1:
                raise ValueError("seg_tag needs one entry per segment")
        tags = seg_tag is not None if tags is None else tags
        if tags and seg_tag is None:
            raise ValueError("tags need seg_tag")
        g = grid.h if grid is not None else None
        s, s2, s3 = L.RetimeSummary(), L.StopsSummary(), L.JerkSummary()

        def call(time_q, w_q, bound, th, sq, tg):
            rc = self.ctx.lib.wa_traj_retime_jerk(g, self.h, C.byref(lim), _ptr(v_limit), _ptr(dwell), C.c_double(tick), int(window),
                                                  _ptr(seg_tag), _ptr(time_q), _ptr(w_q), _ptr(bound), C.byref(th) if th is not None else None,
                                                  _ptr(sq), _ptr(tg), C.byref(s), C.byref(s2), C.byref(s3))
            if rc != 7:   # WA_ERR_CAPACITY: everything but the ticks is there
                self.ctx.check(rc)
            return rc

        sq = tg = None
        if s_q or tags:
            if call(None, None, None, None, None, None) == 0:
                sq = np.empty(int(s3.n_ticks), np.int64) if s_q else None
                tg = np.empty(int(s3.n_ticks), np.uint8) if tags else None
        time_q, w_q, bound = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
        th = C.c_void_p()
        call(time_q, w_q, bound, th if ticks else None, sq, tg)
        summary = {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in L.RetimeSummary._fields_}
        return (time_q, w_q, bound, Trajectory(self.ctx, th) if th.value else None, sq, tg, summary,
                {k: int(getattr(s2, k)) for k, _ in L.StopsSummary._fields_}, {k: int(getattr(s3, k)) for k, _ in L.JerkSummary._fields_})

    def retime_jerk_axes(self, q, v_max, acc, dec, tick, window, dwell=None, seg_tag=None, grid=None, tool=None, near_add=-1,
                         a_lat=float("inf"), v_near=0.0, near_d2=-1, v_limit=None, ticks=True, s_q=False, tags=None, axes=True, blocked=True):
        """wa_traj_retime_jerk_axes: retime_jerk() with one torch axis per filtered tick.  `q`: the quantised sample axes (quantise_axes).
        A moving tick takes the axis of its place on the polyline, interpolated along its segment like tick_axes(); while the filtered
        position rests at a stop the torch turns in place from the first to the last axis of the coincident samples, linear in the
        tick number.  Every axis is checked against `grid` with `tool` at the tick's position (both or neither).
        Returns retime_jerk()'s tuple plus (axes Trajectory or None, blocked uint8[n_ticks] or None, axes dict)."""
        n = len(self)
        q = self._axes(q)
        lim = L.RetimeLimits(v_max, acc, dec, a_lat, v_near, near_d2)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        dwell = self._dwells(dwell, "dwell")
        if seg_tag is not None:
            seg_tag = np.ascontiguousarray(seg_tag, np.uint8).reshape(-1)
            if len(seg_tag) != n - 1:
                raise ValueError("seg_tag needs one entry per segment")
        tags = seg_tag is not None if tags is None else tags
        if tags and seg_tag is None:
            raise ValueError("tags need seg_tag")
        if tool is not None:
            tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        g = grid.h if grid is not None else None
        s, s2, s3, s4 = L.RetimeSummary(), L.StopsSummary(), L.JerkSummary(), L.JerkAxesSummary()

        def call(time_q, w_q, bound, th, sq, tg, ah, bl):
            rc = self.ctx.lib.wa_traj_retime_jerk_axes(g, self.h, C.byref(lim), _ptr(v_limit), _ptr(dwell), C.c_double(tick), int(window),
                                                       _ptr(seg_tag), _ptr(q), C.byref(tool) if tool is not None else None, near_add,
                                                       _ptr(time_q), _ptr(w_q), _ptr(bound), C.byref(th) if th is not None else None,
                                                       _ptr(sq), _ptr(tg), C.byref(ah) if ah is not None else None, _ptr(bl),
                                                       C.byref(s), C.byref(s2), C.byref(s3), C.byref(s4))
            if rc != 7:   # WA_ERR_CAPACITY: everything but the ticks is there
                self.ctx.check(rc)
            return rc

        sq = tg = bl = None
        if s_q or tags or blocked:   # (the host arrays are sized by a first call without outputs: the same bytes on every call)
            if call(None, None, None, None, None, None, None, None) == 0:
                sq = np.empty(int(s3.n_ticks), np.int64) if s_q else None
                tg = np.empty(int(s3.n_ticks), np.uint8) if tags else None
                bl = np.empty(int(s3.n_ticks), np.uint8) if blocked else None
        time_q, w_q, bound = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
        th, ah = C.c_void_p(), C.c_void_p()
        call(time_q, w_q, bound, th if ticks else None, sq, tg, ah if axes else None, bl)
        summary = {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in L.RetimeSummary._fields_}
        return (time_q, w_q, bound, Trajectory(self.ctx, th) if th.value else None, sq, tg, summary,
                {k: int(getattr(s2, k)) for k, _ in L.StopsSummary._fields_}, {k: int(getattr(s3, k)) for k, _ in L.JerkSummary._fields_},
                Trajectory(self.ctx, ah) if ah.value else None, bl, {k: int(getattr(s4, k)) for k, _ in L.JerkAxesSummary._fields_})

    def retime_jerk_frames(self, q, v_max, acc, dec, tick, window, dwell=None, seg_tag=None, grid=None, tool=None, near_add=-1, weave=None,
                           a_lat=float("inf"), v_near=0.0, near_d2=-1, v_limit=None, ticks=True, s_q=False, tags=None, axes=True, blocked=True,
                           lat=True):
        """wa_traj_retime_jerk_frames: retime_jerk_axes() with the lateral of every tick (the direction across the seam: torch axis x
        direction of travel, left of travel with the torch body up) and, with `weave` (make_weave() or its keywords as a dict), a periodic offset along the lateral
        on the segments whose tag matches, tapered at both ends of a run.  The ticks then hold the woven positions and the bead check
        runs where they are.  Returns retime_jerk_axes()'s tuple plus (lat Trajectory or None, frames dict)."""
        n = len(self)
        q = self._axes(q)
        lim = L.RetimeLimits(v_max, acc, dec, a_lat, v_near, near_d2)
        if v_limit is not None:
            v_limit = np.ascontiguousarray(v_limit, np.float32).reshape(-1)
            if len(v_limit) != n:
                raise ValueError("v_limit needs one entry per sample")
        dwell = self._dwells(dwell, "dwell")
        if seg_tag is not None:
            seg_tag = np.ascontiguousarray(seg_tag, np.uint8).reshape(-1)
            if len(seg_tag) != n - 1:
                raise ValueError("seg_tag needs one entry per segment")
        tags = seg_tag is not None if tags is None else tags
        if tags and seg_tag is None:
            raise ValueError("tags need seg_tag")
        if tool is not None:
            tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        if weave is not None and not isinstance(weave, L.Weave):
            weave = make_weave(**weave)
        g = grid.h if grid is not None else None
        s, s2, s3, s4, s5 = L.RetimeSummary(), L.StopsSummary(), L.JerkSummary(), L.JerkAxesSummary(), L.FramesSummary()

        def call(time_q, w_q, bound, th, sq, tg, ah, bl, lh):
            rc = self.ctx.lib.wa_traj_retime_jerk_frames(g, self.h, C.byref(lim), _ptr(v_limit), _ptr(dwell), C.c_double(tick), int(window),
                                                         _ptr(seg_tag), _ptr(q), C.byref(tool) if tool is not None else None, near_add,
                                                         C.byref(weave) if weave is not None else None,
                                                         _ptr(time_q), _ptr(w_q), _ptr(bound), C.byref(th) if th is not None else None,
                                                         _ptr(sq), _ptr(tg), C.byref(ah) if ah is not None else None, _ptr(bl),
                                                         C.byref(lh) if lh is not None else None,
                                                         C.byref(s), C.byref(s2), C.byref(s3), C.byref(s4), C.byref(s5))
            if rc != 7:   # WA_ERR_CAPACITY: everything but the ticks is there
                self.ctx.check(rc)
            return rc

        sq = tg = bl = None
        if s_q or tags or blocked:   # (the host arrays are sized by a first call without outputs: the same bytes on every call)
            if call(None, None, None, None, None, None, None, None, None) == 0:
                sq = np.empty(int(s3.n_ticks), np.int64) if s_q else None
                tg = np.empty(int(s3.n_ticks), np.uint8) if tags else None
                bl = np.empty(int(s3.n_ticks), np.uint8) if blocked else None
        time_q, w_q, bound = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
        th, ah, lh = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call(time_q, w_q, bound, th if ticks else None, sq, tg, ah if axes else None, bl, lh if lat else None)
        summary = {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in L.RetimeSummary._fields_}
        return (time_q, w_q, bound, Trajectory(self.ctx, th) if th.value else None, sq, tg, summary,
                {k: int(getattr(s2, k)) for k, _ in L.StopsSummary._fields_}, {k: int(getattr(s3, k)) for k, _ in L.JerkSummary._fields_},
                Trajectory(self.ctx, ah) if ah.value else None, bl, {k: int(getattr(s4, k)) for k, _ in L.JerkAxesSummary._fields_},
                Trajectory(self.ctx, lh) if lh.value else None, {k: int(getattr(s5, k)) for k, _ in L.FramesSummary._fields_})

    def axis_dwells(self, q, omega, dwell=None):
        """wa_traj_axes_dwells: the dwell every change of direction on a segment without length needs at the turn rate `omega` (chord of
        the unit axes per second), never below the caller's own `dwell` there.  Returns (float64[n-1] for retime_stops(dwell=...),
        summary)."""
        q = self._axes(q)
        dwell = self._dwells(dwell, "dwell")
        out = np.empty(max(len(self) - 1, 0), np.float64)
        s = L.AxesDwellsSummary()
        self.ctx.check(self.ctx.lib.wa_traj_axes_dwells(self.h, _ptr(q), C.c_double(omega), _ptr(dwell), _ptr(out), C.byref(s)))
        return out, {k: (float(s.max_need) if k == "max_need" else int(getattr(s, k))) for k, _ in L.AxesDwellsSummary._fields_}

    def tick_axes_stops(self, q, time_q, w_q, acc, dec, tick, seg_tag=None, grid=None, tool=None, near_add=-1, axes=True, blocked=True):
        """wa_traj_tick_axes_stops: tick_axes() on retime_stops(...)'s result.  During a dwell the torch stays where it is and turns from
        the stop's first axis to its second, linear in time.  seg_tag: one byte per segment (arc on / off, a seam number, whatever the
        caller puts there); every tick gets the tag of its segment.  Returns tick_axes()'s tuple, the tags and the stops summary:
        (Trajectory of n_ticks unit axes or None, blocked uint8[n_ticks] or None, summary, tags uint8[n_ticks] or None, stops dict)."""
        n = len(self)
        q = self._axes(q)
        time_q = np.ascontiguousarray(time_q, np.int64).reshape(-1)
        w_q = np.ascontiguousarray(w_q, np.int64).reshape(-1)
        if len(time_q) != n or len(w_q) != n:
            raise ValueError("time_q and w_q need one entry per sample")
        if seg_tag is not None:
            seg_tag = np.ascontiguousarray(seg_tag, np.uint8).reshape(-1)
            if len(seg_tag) != n - 1:
                raise ValueError("seg_tag needs one entry per segment")
        if tool is not None:
            tool = tool if isinstance(tool, L.ToolBeads) else torch_tool(*tool)
        n_ticks = 0
        if n >= 2:
            tq = int(np.rint(np.float64(tick) * RETIME_Q)) if np.isfinite(tick) else 0
            n_ticks = int(time_q[-1]) // tq + 1 + (1 if int(time_q[-1]) % tq else 0) if tq >= 1 and time_q[-1] >= 0 else 0
            n_ticks = n_ticks if n_ticks <= 1 << 31 else 0
        out = np.empty(n_ticks, np.uint8) if blocked and n >= 2 else None
        tags = np.empty(n_ticks, np.uint8) if seg_tag is not None else None
        th, s, s2 = C.c_void_p(), L.TickAxesSummary(), L.TickStopsSummary()
        self.ctx.check(self.ctx.lib.wa_traj_tick_axes_stops(grid.h if grid is not None else None, self.h, _ptr(q),
                                                            C.byref(tool) if tool is not None else None, near_add, C.c_double(acc), C.c_double(dec),
                                                            C.c_double(tick), _ptr(time_q), _ptr(w_q), _ptr(seg_tag), C.byref(th) if axes else None,
                                                            _ptr(out), _ptr(tags), C.byref(s), C.byref(s2)))
        summary = {k: int(getattr(s, k)) for k, _ in L.TickAxesSummary._fields_}
        return (Trajectory(self.ctx, th) if th.value else None, out, summary, tags,
                {k: int(getattr(s2, k)) for k, _ in L.TickStopsSummary._fields_})

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.wa_traj_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Bspline:
    """BS_Basic<float, dim, degree, level_ini, level_fin> (core/BSplineBasic.h) on the device."""

    def __init__(self, ctx, dim, degree, level_ini, level_fin, n_middle, uninit_bits=0):
        self.ctx, self.dim, self.degree, self.n_middle = ctx, dim, degree, n_middle
        h = C.c_void_p()
        ctx.check(ctx.lib.wa_bspline_create(ctx.h, dim, degree, level_ini, level_fin, n_middle, C.byref(h)))
        self.h = h
        ctx._children.add(self)
        if uninit_bits:
            ctx.check(ctx.lib.wa_bspline_set_uninit(self.h, uninit_bits))

    @classmethod
    def adopt(cls, ctx, handle, dim, degree, n_middle):
        """a wa_bspline the library created (wa_grid_fit_trajectory); owned and destroyed by the wrapper like any other"""
        b = cls.__new__(cls)
        b.ctx, b.dim, b.degree, b.n_middle, b.h = ctx, dim, degree, n_middle, handle
        ctx._children.add(b)
        return b

    def set_param(self, init, fin, middle, fin_time):
        """SetParam; `middle` is an (n_middle, stride >= dim) array or a Trajectory."""
        init = np.ascontiguousarray(init, np.float32)
        fin = np.ascontiguousarray(fin, np.float32)
        if isinstance(middle, Trajectory):
            rc = self.ctx.lib.wa_bspline_set_param_traj(self.h, _ptr(init), _ptr(fin), middle.h, C.c_float(fin_time))
        else:
            middle = np.ascontiguousarray(middle, np.float32)
            middle = middle.reshape(self.n_middle, -1) if middle.size else np.zeros((0, self.dim), np.float32)
            rc = self.ctx.lib.wa_bspline_set_param(self.h, _ptr(init), _ptr(fin), _ptr(middle), middle.shape[1],
                                                   C.c_float(fin_time))
        self.ctx.check(rc)

    def arrays(self):
        nk, nc = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.wa_bspline_info(self.h, C.byref(nk), C.byref(nc)))
        knots, cps = np.empty(nk.value, np.float32), np.empty((nc.value, self.dim), np.float32)
        self.ctx.check(self.ctx.lib.wa_bspline_read(self.h, _ptr(knots), _ptr(cps)))
        return knots, cps

    def eval(self, us, der=0):
        us = np.ascontiguousarray(us, np.float32).reshape(-1)
        out = np.empty((len(us), self.dim), np.float32)
        ok = np.empty(len(us), np.uint8)
        self.ctx.check(self.ctx.lib.wa_bspline_eval(self.h, _ptr(us), len(us), der, _ptr(out), _ptr(ok)))
        return out, ok

    def eval_host(self, u, der=0):
        """one time on the host (wa_bspline_eval_host): (dim values, ok)"""
        out = np.zeros(self.dim, np.float32)
        ok = C.c_uint8()
        self.ctx.check(self.ctx.lib.wa_bspline_eval_host(self.h, C.c_float(u), der, _ptr(out), C.byref(ok)))
        return out, bool(ok.value)

    def sample(self, t0, dt, count, der=0, host=True, device=False):
        out = np.empty((count, self.dim), np.float32) if host else None
        ok = np.empty(count, np.uint8) if host else None
        th = C.c_void_p()
        self.ctx.check(self.ctx.lib.wa_bspline_sample(self.h, C.c_float(t0), C.c_float(dt), count, der, _ptr(out),
                                                      _ptr(ok), C.byref(th) if device else None))
        traj = Trajectory(self.ctx, th) if device else None
        return (out, ok, traj) if device else (out, ok)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.wa_bspline_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def gtsp_solve(ctx, dist, cnt=None, mode=RNG_DEV, seed=1, stream=0, max_iterations=0, rand_state=None, want_pher=False):
    dist = np.ascontiguousarray(dist, np.float64)
    if dist.ndim == 2:
        dist = dist[None]
    inst, n = dist.shape[0], dist.shape[1]
    cnt = n * (n - 1) // 2 if cnt is None else cnt
    p = GtspParams(mode, seed, stream, max_iterations)
    edges = np.zeros((inst, n, 2), np.int32)
    cost = np.zeros(inst, np.float64)
    iters = np.zeros(inst, np.int32)
    pher = np.zeros((inst, n, n), np.float64) if want_pher else None
    st = None if rand_state is None else np.ascontiguousarray(rand_state, np.int32)
    ctx.check(ctx.lib.wa_gtsp_solve(ctx.h, _ptr(dist), n, cnt, inst, C.byref(p), _ptr(st), _ptr(edges), _ptr(cost),
                                    _ptr(iters), _ptr(pher)))
    return dict(edges=edges, L=cost, iters=iters, pher=pher, rand_state=st)


SEAM_Q = 1 << 20   # quanta per unit of cost in wa_gtsp_seam_tour's integers


def seam_tour(ctx, dist, closed=True, or_len=3, n_starts=64, max_passes=1 << 20, seed=1, order0=None, dir0=None):
    """wa_gtsp_seam_tour: order and direction of m two-ended seams from the 2m x 2m endpoint costs (seam s: endpoints 2s, 2s+1) by a
    multi-start local search; dir[k] = 0 enters seam order[k] at its even endpoint (Trajectory.stitch's reverse flag is dir[k] = 1)"""
    dist = np.ascontiguousarray(dist, np.float64)
    m = dist.shape[0] // 2
    assert dist.shape == (2 * m, 2 * m), "dist is 2m x 2m"
    p = L.SeamParams(1 if closed else 0, or_len, n_starts, max_passes, seed)
    order0 = None if order0 is None else np.ascontiguousarray(order0, np.int32)
    dir0 = None if dir0 is None else np.ascontiguousarray(dir0, np.uint8)
    assert (order0 is None or order0.shape == (m,)) and (dir0 is None or dir0.shape == (m,)), "order0 / dir0 hold m entries"
    order, dirs = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    n = max(int(n_starts), 0)
    costs, passes = np.zeros(n, np.int64), np.zeros(n, np.int32)
    s = L.SeamSummary()
    ctx.check(ctx.lib.wa_gtsp_seam_tour(ctx.h, _ptr(dist), m, C.byref(p), _ptr(order0), _ptr(dir0), _ptr(order), _ptr(dirs), _ptr(costs),
                                   _ptr(passes), C.byref(s)))
    summary = {k: int(getattr(s, k)) for k, _ in L.SeamSummary._fields_}
    return dict(order=order, dir=dirs, cost_q=summary["cost_q"], cost=summary["cost_q"] / SEAM_Q, start_cost_q=costs, start_passes=passes,
                summary=summary)


def seam_tour_exact(ctx, dist, closed=True):
    """wa_gtsp_seam_tour_exact: the optimal order and directions, up to 16 seams (15 when open)"""
    dist = np.ascontiguousarray(dist, np.float64)
    m = dist.shape[0] // 2
    assert dist.shape == (2 * m, 2 * m), "dist is 2m x 2m"
    order, dirs, cost = np.zeros(m, np.int32), np.zeros(m, np.uint8), C.c_int64(0)
    ctx.check(ctx.lib.wa_gtsp_seam_tour_exact(ctx.h, _ptr(dist), m, 1 if closed else 0, _ptr(order), _ptr(dirs), C.byref(cost)))
    return dict(order=order, dir=dirs, cost_q=int(cost.value), cost=cost.value / SEAM_Q)


def _seam_rules(m, before, after, fixed):
    """the rule arrays of the seam-tour calls as the library reads them: (before, after, n_prec, fixed)"""
    before = np.ascontiguousarray([] if before is None else before, np.int32).reshape(-1)
    after = np.ascontiguousarray([] if after is None else after, np.int32).reshape(-1)
    assert before.shape == after.shape, "one `after` seam per `before` seam"
    fixed = None if fixed is None else np.ascontiguousarray(fixed, np.uint8)
    assert fixed is None or fixed.shape == (m,), "fixed holds m bytes"
    return (before if len(before) else None), (after if len(after) else None), len(before), fixed


def seam_tour_rules(ctx, dist, before=None, after=None, fixed=None, closed=True, or_len=3, n_starts=64, max_passes=1 << 20, seed=1,
                    order0=None, dir0=None):
    """wa_gtsp_seam_tour_rules: seam_tour under job rules.  Seam before[k] is welded earlier than seam after[k]; fixed[s] = 1 / 2 enters
    seam s at its even / odd endpoint only.  The tour is read from seam 0 when closed (nothing may go before it) and from its first
    seam when open; a given order0 / dir0 must keep the rules."""
    dist = np.ascontiguousarray(dist, np.float64)
    m = dist.shape[0] // 2
    assert dist.shape == (2 * m, 2 * m), "dist is 2m x 2m"
    before, after, n_prec, fixed = _seam_rules(m, before, after, fixed)
    p = L.SeamParams(1 if closed else 0, or_len, n_starts, max_passes, seed)
    order0 = None if order0 is None else np.ascontiguousarray(order0, np.int32)
    dir0 = None if dir0 is None else np.ascontiguousarray(dir0, np.uint8)
    assert (order0 is None or order0.shape == (m,)) and (dir0 is None or dir0.shape == (m,)), "order0 / dir0 hold m entries"
    order, dirs = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    n = max(int(n_starts), 0)
    costs, passes = np.zeros(n, np.int64), np.zeros(n, np.int32)
    s = L.SeamRulesSummary()
    ctx.check(ctx.lib.wa_gtsp_seam_tour_rules(ctx.h, _ptr(dist), m, C.byref(p), _ptr(before), _ptr(after), n_prec, _ptr(fixed), _ptr(order0),
                                              _ptr(dir0), _ptr(order), _ptr(dirs), _ptr(costs), _ptr(passes), C.byref(s)))
    summary = {k: int(getattr(s, k)) for k, _ in L.SeamRulesSummary._fields_}
    return dict(order=order, dir=dirs, cost_q=summary["cost_q"], cost=summary["cost_q"] / SEAM_Q, start_cost_q=costs, start_passes=passes,
                summary=summary)


def seam_tour_rules_exact(ctx, dist, before=None, after=None, fixed=None, closed=True):
    """wa_gtsp_seam_tour_rules_exact: the optimal admissible order and directions, up to 16 seams (15 when open)"""
    dist = np.ascontiguousarray(dist, np.float64)
    m = dist.shape[0] // 2
    assert dist.shape == (2 * m, 2 * m), "dist is 2m x 2m"
    before, after, n_prec, fixed = _seam_rules(m, before, after, fixed)
    order, dirs, cost = np.zeros(m, np.int32), np.zeros(m, np.uint8), C.c_int64(0)
    ctx.check(ctx.lib.wa_gtsp_seam_tour_rules_exact(ctx.h, _ptr(dist), m, 1 if closed else 0, _ptr(before), _ptr(after), n_prec, _ptr(fixed),
                                                    _ptr(order), _ptr(dirs), C.byref(cost)))
    return dict(order=order, dir=dirs, cost_q=int(cost.value), cost=cost.value / SEAM_Q)


def seam_rules_check(order, dirs, before=None, after=None, fixed=None, closed=True, ctx=None):
    """wa_gtsp_seam_rules_check (host only, a context is optional): (given pairs out of order, one-way seams entered at the wrong end) of a
    tour"""
    order, dirs = np.ascontiguousarray(order, np.int32), np.ascontiguousarray(dirs, np.uint8)
    m = len(order)
    assert order.shape == (m,) and dirs.shape == (m,), "order / dir hold m entries"
    before, after, n_prec, fixed = _seam_rules(m, before, after, fixed)
    bad_p, bad_d = C.c_int64(0), C.c_int64(0)
    rc = (ctx.lib if ctx is not None else L.load()).wa_gtsp_seam_rules_check(ctx.h if ctx is not None else None, m, 1 if closed else 0, _ptr(before), _ptr(after), n_prec, _ptr(fixed), _ptr(order), _ptr(dirs),
                                                    C.byref(bad_p), C.byref(bad_d))
    if rc:
        raise ValueError("wa_gtsp_seam_rules_check: the rules or the tour are not well-formed (status %d)" % rc)
    return int(bad_p.value), int(bad_d.value)


def jerk_window(acc, dec, jerk, tick):
    """wa_traj_jerk_window (host only): the window, in ticks, of Trajectory.retime_jerk that bounds the jerk along the path by `jerk`
    under the ramps acc / dec: max(1, ceil(2 * max(acc, dec) / (jerk * tick)))"""
    w = C.c_int32(0)
    rc = L.load().wa_traj_jerk_window(None, C.c_double(acc), C.c_double(dec), C.c_double(jerk), C.c_double(tick), C.byref(w))
    if rc:
        raise ValueError("wa_traj_jerk_window: acc, dec, jerk and tick must be finite and > 0, the window at most 2^20 ticks (status %d)" % rc)
    return int(w.value)


def weave_pattern(kind, P):
    """one period of a weave as the int16 table of wa_weave (P entries in -16384 .. 16384, entry 0 is 0, the table is interpolated
    linearly and wraps): "triangle" (0, +1 at a quarter, -1 at three quarters), "sine", or "trapezoid" (a triangle of twice the height
    cut at +-1: the torch lingers at both toes of the weld).  numpy on the host; the table is the caller's data and may be anything."""
    P = int(P)
    if not 2 <= P <= 4096:
        raise ValueError("a pattern has 2 .. 4096 entries")
    u = np.arange(P, dtype=np.float64) / P
    tri = np.where(u < 0.25, 4.0 * u, np.where(u < 0.75, 2.0 - 4.0 * u, 4.0 * u - 4.0))
    if kind == "triangle":
        w = tri
    elif kind == "sine":
        w = np.sin(2.0 * np.pi * u)
    elif kind == "trapezoid":
        w = np.clip(2.0 * tri, -1.0, 1.0)
    else:
        raise ValueError("kind is 'triangle', 'sine' or 'trapezoid'")
    out = np.rint(w * 16384.0).astype(np.int16)
    out[0] = 0
    return out


def make_weave(amplitude, wavelength, pattern, taper=0.0, tag_mask=0xff, tag_value=1):
    """a wa_weave for Trajectory.retime_jerk_frames: an offset of at most `amplitude` along the lateral, one period of `pattern`
    (weave_pattern) per `wavelength` of arc length, on every segment with (seg_tag & tag_mask) == tag_value, rising from 0 over `taper`
    at both ends of a run of such segments"""
    pattern = np.ascontiguousarray(pattern, np.int16).reshape(-1)
    w = L.Weave(float(amplitude), float(wavelength), float(taper), pattern.ctypes.data, len(pattern), int(tag_mask), int(tag_value))
    w._pattern = pattern   # (the table lives as long as the structure)
    return w


TORCH_INF = L.TORCH_INF   # leg cost of a one-sample leg whose two pins differ (wa_traj_tool_axes, rule 5)


def torch_tool(dist16, r2):
    """the beads of a torch body for Trajectory.torch_axes / torch_check: bead j sits dist16[j] sixteenths of a voxel behind the tip and
    must keep a squared clearance (voxel-index units) above r2[j]"""
    dist16, r2 = np.asarray(dist16, np.int64).reshape(-1), np.asarray(r2, np.int64).reshape(-1)
    if len(dist16) != len(r2) or not 1 <= len(r2) <= L.TORCH_MAX_BEADS:
        raise ValueError("a tool has 1 .. %d beads, one dist16 and one r2 each" % L.TORCH_MAX_BEADS)
    if dist16.min() < -2 ** 31 or dist16.max() >= 2 ** 31 or r2.min() < -2 ** 31 or r2.max() >= 2 ** 31:
        raise ValueError("dist16 and r2 are int32")
    t = L.ToolBeads()
    t.n_beads = len(r2)
    for j in range(len(r2)):
        t.dist16[j], t.r2[j] = int(dist16[j]), int(r2[j])
    return t


class PoseCosts:
    """a wa_pose_costs (`c`) together with the penalty array it points to (`pen`, None for none)"""

    def __init__(self, c, pen):
        self.c, self.pen = c, pen


def pose_costs(hop, bands, turn_costs, pen=None):
    """the cost description of Grid.pose_weighted_*: a step costs `hop` (1 .. 8), plus turn_costs[c] where c is the number of `bands`
    (ascending thresholds on the turn measure U, at most 4) its change of direction exceeds -- turn_costs has one entry more than
    bands, starts with 0 and does not decrease, each at most 15 -- plus pen[v] of the voxel entered (uint8 [n], at most 15 on free
    voxels; Grid.torch_penalties, or Grid.clearance_costs minus 1).  The ranges are checked by the library."""
    bands = np.asarray(bands, np.int64).reshape(-1)
    turn_costs = np.asarray(turn_costs, np.int64).reshape(-1)
    if len(bands) > L.POSE_MAX_BANDS or len(turn_costs) != len(bands) + 1:
        raise ValueError("at most %d bands, and one turn cost more than bands" % L.POSE_MAX_BANDS)
    if max(abs(int(hop)), np.abs(bands).max(initial=0), np.abs(turn_costs).max()) >= 2 ** 31:
        raise ValueError("hop, bands and turn_costs are int32")
    c = L.PoseCosts()
    c.hop_cost, c.n_bands = int(hop), len(bands)
    for b in range(len(bands)):
        c.turn_band[b] = int(bands[b])
    for b in range(len(turn_costs)):
        c.turn_cost[b] = int(turn_costs[b])
    if pen is not None:
        pen = np.ascontiguousarray(pen, np.uint8).reshape(-1)
        c.pen = pen.ctypes.data
    return PoseCosts(c, pen)


class PoseDiagCosts:
    """a wa_pose_diag_costs (`c`) together with the penalty array it points to (`pen`, None for none)"""

    def __init__(self, c, pen):
        self.c, self.pen = c, pen


def pose_diag_costs(step, bands, turn_costs, pen=None):
    """the cost description of Grid.pose_diag_*: `step` = the cost of a face, an edge and a corner move (each 1 .. 16; 3, 4, 5 is the
    usual chamfer); bands, turn_costs and pen as for pose_costs, the turn costs charged on face moves (a diagonal move keeps the
    direction).  The ranges are checked by the library."""
    step = np.asarray(step, np.int64).reshape(-1)
    bands = np.asarray(bands, np.int64).reshape(-1)
    turn_costs = np.asarray(turn_costs, np.int64).reshape(-1)
    if len(step) != 3:
        raise ValueError("step holds three costs: face, edge, corner")
    if len(bands) > L.POSE_MAX_BANDS or len(turn_costs) != len(bands) + 1:
        raise ValueError("at most %d bands, and one turn cost more than bands" % L.POSE_MAX_BANDS)
    if max(np.abs(step).max(), np.abs(bands).max(initial=0), np.abs(turn_costs).max()) >= 2 ** 31:
        raise ValueError("step, bands and turn_costs are int32")
    c = L.PoseDiagCosts()
    c.n_bands = len(bands)
    for i in range(3):
        c.step[i] = int(step[i])
    for b in range(len(bands)):
        c.turn_band[b] = int(bands[b])
    for b in range(len(turn_costs)):
        c.turn_cost[b] = int(turn_costs[b])
    if pen is not None:
        pen = np.ascontiguousarray(pen, np.uint8).reshape(-1)
        c.pen = pen.ctypes.data
    return PoseDiagCosts(c, pen)


def quantise_axes(dirs):
    """rule 1 of the tool section in numpy: float triples (tip -> body) to the integers the axis calls exchange,
    q_c = rint((c / len) * 16384) with len = sqrt((x*x + y*y) + z*z) in float64 on the fp32 components.  Keep the integers: quantising
    q / 16384 a second time can move a component by 1."""
    d = np.asarray(dirs, np.float32).reshape(-1, 3).astype(np.float64)
    if not np.isfinite(d).all():
        raise ValueError("a direction is not finite")
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if not (ln > 0).all():
        raise ValueError("a direction has zero length")
    return np.rint((d / ln[:, None]) * 16384.0).astype(np.int32)


def torch_cone(K, half_angle, axis=(0.0, 0.0, 1.0)):
    """K unit directions on the spherical cap of `half_angle` radians around `axis`, a Fibonacci spiral from the axis outwards
    (direction 0 is the axis itself).  The floats are INPUTS of wa_traj_tool_axes, which quantises them: not part of the bit contract."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    helper = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(a, helper)
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    k = np.arange(K, dtype=np.float64)
    cos_t = 1.0 - (1.0 - np.cos(half_angle)) * (k / max(K - 1, 1))
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = cos_t[:, None] * a + (sin_t * np.cos(phi))[:, None] * u + (sin_t * np.sin(phi))[:, None] * v
    return np.ascontiguousarray(d, np.float32)
