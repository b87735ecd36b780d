#!/usr/bin/env python3
"""Time wa_grid_pose_fit_trajectory beside wa_grid_fit_trajectory on the same polyline, and beside the same loop composed from the calls
that existed before it plus a host check.  Two tours from examples/plan_batch.py's planners, as tools/fit_time.py takes them:
  (a) 96^3 synth_grid, 16 points, --safe-paths 3, 6 001 samples
  (b) 256^3 synth_grid, 64 points, --exact-paths (C5's tour), 100 001 samples
The tour's lattice paths get the lowest open direction of every node's voxel (0 where none is open; K = 64 directions and the 24-bead
torch of examples/plan_batch.py), as tools/pose_shortcut_time.py does, are shortened by wa_grid_pose_shortcut at span 128 and stitched
in tour direction with their holds.  Per tour, at a control spacing of 1 voxel and of 8 voxels:
  - the new call;
  - wa_grid_fit_trajectory on the same polyline, and the new call with identity (a)'s tool (one bead, dist16 0, r2 0, every unheld leg
    given hold 0): the same rounds and bytes, so the difference is the price of the masks and of the mask walk;
  - (tour (a) only) the composed loop: numpy for the pieces, the polygon, the candidates, the blame and the levels; api.Bspline.set_param
    / .sample and Trajectory.clearance for the fit and the voxels; Grid.torch_reach for the masks, once per call; the covers walked on
    the host.
Whole calls, HIP events on the context's stream, one warm-up, median and range of 10.  Kernel times: run it alone under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/pose_fit_time.py --reps 3`.

    python tools/pose_fit_time.py [--reps N] [--only a|b]"""
import ctypes as C
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else "ab"
K, SPAN = 64, 128
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
stream = C.c_void_p(ctx.stream)
ev = [C.c_void_p(), C.c_void_p()]
assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0


def timed(fn):
    out, times = None, []
    for r in range(reps + 1):          # the first call warms up
        ctx.sync()
        hip.hipEventRecord(ev[0], stream)
        out = fn()
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        if r:
            times.append(ms.value)
    return out, "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(times), min(times), max(times), reps)


def lowest_open(mask, p):
    """per node the lowest open direction of its voxel, 0 where none is open"""
    k = np.zeros(len(p), np.int32)
    todo = np.ones(len(p), bool)
    for w in range(mask.shape[0]):
        m = mask[w, p]
        low = m & (~m + np.uint64(1))
        hit = todo & (m != 0)
        k[hit] = w * 64 + np.log2(low[hit].astype(np.float64)).astype(np.int32)
        todo &= ~hit
    return k


def tour_polyline(n, P, safe):
    """(grid, dirs, tool, stitched waypoints as a Trajectory, holds per leg)"""
    free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
    grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, P, seed=7)
    cost, paths, _ = pb.plan_safe(grid, pts, 3, shortcut=SPAN) if safe else pb.plan_exact(grid, pts, shortcut=SPAN)
    tour = api.gtsp_solve(ctx, cost, mode=api.RNG_DEV, seed=7)
    edges = tour["edges"][0][:-1]
    segs = [np.asarray(paths[(min(a, b), max(a, b))], np.int64) for a, b in edges]
    rev = [1 if a > b else 0 for a, b in edges]
    tool, dirs, _ = pb.torch_tool_and_cone(grid, K)
    mask, _, reach = grid.torch_reach(dirs, tool)
    wps, _, holds, _, summ = api.pose_shortcut_paths(grid, dirs, tool, -1, segs, [lowest_open(mask, s) for s in segs], SPAN)
    parts = []
    for h, r in zip(holds, rev):
        parts += [np.asarray(h[::-1] if r else h, np.int32), np.full(1, -1, np.int32)]
    print("  reach:", reach, "\n  pose shortcut of the tour's %d paths:" % len(segs), summ)
    return grid, dirs, tool, api.Trajectory.stitch(grid, wps, rev), np.concatenate(parts)[:-1]


# ---- the definition's host-side steps (include/weldacs.h), for the composed loop
def pieces(xyz, levels, spacing):
    p = xyz.astype(np.float64)
    d = p[1:] - p[:-1]
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    c = np.ceil((ln * np.float64(2.0) ** levels) / np.float64(np.float32(spacing)))
    return np.where(c >= 1.0, c, 1.0).astype(np.int64)


def polygon(xyz, m):
    leg = np.repeat(np.arange(len(m)), m)
    j = (np.arange(m.sum()) - np.repeat(np.cumsum(m) - m, m)).astype(np.float32)
    t = j / np.repeat(m, m).astype(np.float32)
    pts = xyz[leg] + ((xyz[leg + 1] - xyz[leg]) * t[:, None]).astype(np.float32)
    return np.vstack([pts, xyz[-1:]]).astype(np.float32), np.concatenate([leg, [len(m) - 1]])


def cover(dims, a, b):
    """raster ids of the supercover between voxels a and b: the voxels of their box whose per-axis intervals of t share a point of [0, 1]"""
    nx, ny, _ = dims
    pa = np.array([a % nx, (a // nx) % ny, a // (nx * ny)], np.int64)
    pb_ = np.array([b % nx, (b // nx) % ny, b // (nx * ny)], np.int64)
    d = pb_ - pa
    box = np.stack(np.meshgrid(*[np.arange(min(p, q), max(p, q) + 1) for p, q in zip(pa, pb_)], indexing="ij"), -1).reshape(-1, 3)
    lo_n, lo_d, hi_n, hi_d = np.zeros(len(box), np.int64), np.ones(len(box), np.int64), np.ones(len(box), np.int64), np.ones(len(box), np.int64)
    for c in range(3):
        if d[c] == 0:
            continue
        e1, e2 = 2 * (box[:, c] - pa[c]) - 1, 2 * (box[:, c] - pa[c]) + 1
        if d[c] < 0:
            e1, e2 = -e2, -e1
        den = 2 * abs(int(d[c]))
        up = e1 * lo_d > lo_n * den
        lo_n, lo_d = np.where(up, e1, lo_n), np.where(up, den, lo_d)
        dn = e2 * hi_d < hi_n * den
        hi_n, hi_d = np.where(dn, e2, hi_n), np.where(dn, den, hi_d)
    keep = lo_n * hi_d <= hi_n * lo_d
    v = box[keep]
    return (v[:, 2] * ny + v[:, 1]) * nx + v[:, 0]


def composed(grid, dirs, tool, xyz, holds, degree, spacing, max_level, n_samples, stats=None):
    mask, _, _ = grid.torch_reach(dirs, tool)                    # once per call, as the call itself recomputes them
    dims = (grid.nx, grid.ny, grid.nz)
    levels = np.zeros(len(xyz) - 1, np.int64)
    z = np.zeros((degree - 1, 3), np.float32)
    opened = lambda v, c: (mask[c >> 6, v] >> np.uint64(c & 63)) & np.uint64(1)   # noqa: E731
    for rnd in range(32):
        pts, leg = polygon(xyz, pieces(xyz, levels, spacing))
        own = np.concatenate([np.full(degree - 1, leg[0]), leg, np.full(degree - 1, leg[-1])])
        b = api.Bspline(ctx, 3, degree, degree - 1, degree - 1, len(pts) - 2)
        ft = np.float32(len(pts) - 2 + degree)
        b.set_param(np.vstack([pts[:1], z]), np.vstack([pts[-1:], z]), pts[1:-1], ft)
        dt = ft / np.float32(n_samples - 1)
        _, _, traj = b.sample(0.0, dt, n_samples, host=False, device=True)
        ids, _, hits, _ = traj.clearance(grid)
        knots, cps = b.arrays()
        # knots are the integers i - D: the span of u is D + floor(u), the last span for u at the end
        u = np.minimum(np.arange(n_samples).astype(np.float32) * dt, ft)
        span = np.minimum(np.floor(u).astype(np.int64), int(ft) - 1) + degree
        hs = holds[own[span[:, None] - degree + np.arange(degree + 1)[None, :]]]          # n_samples, D + 1
        slots = np.concatenate([hs[:-1], hs[1:]], 1)                                      # n_seg, 2 (D + 1)
        blocked = np.zeros(n_samples - 1, bool)
        for i in range(n_samples - 1):
            cand = []
            for h in slots[i]:
                if h >= 0 and h not in cand:
                    cand.append(int(h))
            if not cand:
                blocked[i] = hits[i]
            elif ids[i] == ids[i + 1]:
                blocked[i] = not any(opened(ids[i], c) for c in cand)
            else:
                cv = cover(dims, int(ids[i]), int(ids[i + 1]))
                blocked[i] = not any(opened(cv, c).all() for c in cand)
        mark = np.zeros(len(levels), bool)
        h = np.flatnonzero(blocked)
        if len(h):
            for e in (h, h + 1):
                for q in range(degree + 1):
                    mark[own[span[e] - degree + q]] = True
        rise = mark & (levels < max_level)
        if stats is not None:
            stats.append((len(cps), int(blocked.sum())))
        traj.close()
        b.close()
        if not blocked.any() or not rise.any() or rnd == 31:
            return knots, cps, levels, rnd + 1, int(blocked.sum())
        levels[rise] += 1


point = api.torch_tool([0], [0])
for tag, n, P, safe, n_samples in (("a", 96, 16, True, 6001), ("b", 256, 64, False, 100001)):
    if tag not in only:
        continue
    print("(%s) %d^3, %d points, %d samples" % (tag, n, P, n_samples))
    grid, dirs, tool, poly, holds = tour_polyline(n, P, safe)
    xyz = poly.points()
    print("  polyline of %d points, %d of its %d legs held, %d of zero length" % (len(xyz), (holds >= 0).sum(), len(holds),
                                                                                  (np.abs(np.diff(xyz, axis=0)).sum(1) == 0).sum()))
    held = np.where(holds >= 0, holds, 0).astype(np.int32)
    for voxels in (1.0, 8.0):
        spacing = float(np.float32(voxels) * np.float32(grid.precision))

        def pose(t=tool, h=holds):
            b, samples, levels, seg_dir, blocked, s = poly.pose_fit(grid, dirs, t, h, 3, spacing, 6, n_samples)
            k = b.arrays()
            b.close()
            samples.close()
            return k, levels, s

        def plain():
            b, samples, levels, s = poly.fit(grid, 3, spacing, 6, n_samples)
            k = b.arrays()
            b.close()
            samples.close()
            return k, levels, s

        (pk, plev, ps), t_pose = timed(pose)
        (fk, flev, fs), t_plain = timed(plain)
        (ik, ilev, is_), t_ident = timed(lambda: pose(point, held))
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(fk, ik)) and np.array_equal(flev, ilev) \
            and (is_["rounds"], is_["n_blocked_first"], is_["final"]) == (fs["rounds"], fs["n_hit_first"], fs["final"])
        print("  spacing %g voxel(s):" % voxels)
        print("    wa_grid_pose_fit_trajectory: %s" % t_pose)
        print("      ", {k: v for k, v in ps.items() if k != "final"}, ps["final"])
        print("    wa_grid_fit_trajectory:      %s; rounds %d, n_hit %d -> %d, %d control points"
              % (t_plain, fs["rounds"], fs["n_hit_first"], fs["final"]["n_hit"], fs["n_cps"]))
        print("    new call, identity (a)'s tool: %s; same bytes as wa_grid_fit_trajectory: %s" % (t_ident, same))
        if tag == "a":
            stats = []
            composed(grid, dirs, tool, xyz, holds, 3, spacing, 6, n_samples, stats)
            (ck, cc, clev, rounds, nb), t_comp = timed(lambda: composed(grid, dirs, tool, xyz, holds, 3, spacing, 6, n_samples))
            ok = np.array_equal(pk[0].view(np.uint32), ck.view(np.uint32)) and np.array_equal(pk[1].view(np.uint32), cc.view(np.uint32))
            print("    composed loop, %d rounds %s: %s; same spline: %s" % (rounds, stats, t_comp, ok))
    poly.close()
    grid.close()
