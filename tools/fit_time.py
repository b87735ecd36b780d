#!/usr/bin/env python3
"""Time wa_grid_fit_trajectory against the same loop composed from the calls that existed before it (numpy for the pieces, the control
polygon, the blame and the levels; api.Bspline.set_param / .sample and Trajectory.clearance for the fit and the check: per round the
middle points go in, the knots, the control points and the hit flags come out).  Two plans from examples/plan_batch.py:
  (a) 96^3 synth_grid, 16 points, --safe-paths 3 --shortcut, 6 001 samples
  (b) 256^3 synth_grid, 64 points, --exact-paths --shortcut (span 128), 100 001 samples
each at a control spacing of 1 voxel and of 8 voxels (where the loop has work to do).  Whole calls, HIP events on the context's
stream, one warm-up, median and range.  Kernel times: run it alone under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fit_time.py --reps 3`.

    python tools/fit_time.py [--reps N] [--only a|b]"""
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


def composed(grid, xyz, degree, spacing, max_level, n_samples, stats=None):
    levels = np.zeros(len(xyz) - 1, np.int64)
    z = np.zeros((degree - 1, 3), np.float32)
    for rnd in range(32):
        pts, leg = polygon(xyz, pieces(xyz, levels, spacing))
        own = np.concatenate([np.full(degree - 1, leg[0]), leg, np.full(degree - 1, leg[-1])])
        b = api.Bspline(ctx, 3, degree, degree - 1, degree - 1, len(pts) - 2)
        ft = np.float32(len(pts) - 2 + degree)
        b.set_param(np.vstack([pts[:1], z]), np.vstack([pts[-1:], z]), pts[1:-1], ft)
        dt = ft / np.float32(n_samples - 1)
        _, _, traj = b.sample(0.0, dt, n_samples, host=False, device=True)
        _, _, hits, summ = traj.clearance(grid)
        knots, cps = b.arrays()
        mark = np.zeros(len(levels), bool)
        h = np.flatnonzero(hits)
        if len(h):      # knots are the integers i - D: the span of u is D + floor(u), the last span for u at the end
            u = np.minimum(np.concatenate([h, h + 1]).astype(np.float32) * dt, ft)
            span = np.minimum(np.floor(u).astype(np.int64), int(ft) - 1) + degree
            for q in range(degree + 1):
                mark[own[span - degree + q]] = True
        rise = mark & (levels < max_level)
        if stats is not None:
            stats.append((len(cps), summ["n_hit"]))
        traj.close()
        b.close()
        if summ["n_hit"] == 0 or not rise.any() or rnd == 31:
            return knots, cps, levels, rnd + 1, summ
        levels[rise] += 1


def waypoint_polyline(n, P, safe):
    free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
    grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    pts = synth.synth_weld_points(free, n, P, seed=7)
    cost, paths, _ = pb.plan_safe(grid, pts, 3, shortcut=128) if safe else pb.plan_exact(grid, pts, shortcut=128)
    short = pb.plan.last_shortcut
    tour = api.gtsp_solve(ctx, cost, mode=api.RNG_DEV, seed=7)
    edges = tour["edges"][0][:-1]
    wsegs = [short[(min(a, b), max(a, b))] for a, b in edges]
    rev = [1 if a > b else 0 for a, b in edges]
    return grid, api.Trajectory.stitch(grid, wsegs, rev)


for tag, n, P, safe, n_samples in (("a", 96, 16, True, 6001), ("b", 256, 64, False, 100001)):
    if tag not in only:
        continue
    grid, poly = waypoint_polyline(n, P, safe)
    xyz = poly.points()
    plen = float(np.linalg.norm(np.diff(xyz.astype(np.float64), axis=0), axis=1).sum())
    print("(%s) %d^3, %d points: polyline of %d points, %.2f m, %d samples" % (tag, n, P, len(xyz), plen, n_samples))
    for voxels in (1.0, 8.0):
        spacing = float(np.float32(voxels) * np.float32(grid.precision))

        def fused():
            b, samples, levels, s = poly.fit(grid, 3, spacing, 6, n_samples)
            k = b.arrays()
            b.close()
            samples.close()
            return k, levels, s

        (fk, flev, fs), t_fused = timed(fused)
        stats = []
        composed(grid, xyz, 3, spacing, 6, n_samples, stats)
        (ck, cc, clev, rounds, csum), t_comp = timed(lambda: composed(grid, xyz, 3, spacing, 6, n_samples))
        same = np.array_equal(fk[0].view(np.uint32), ck.view(np.uint32)) and np.array_equal(fk[1].view(np.uint32), cc.view(np.uint32))
        b, samples, _, _ = poly.fit(grid, 3, spacing, 6, n_samples)
        tlen = float(np.linalg.norm(np.diff(samples.points().astype(np.float64), axis=0), axis=1).sum())
        print("  spacing %g voxel(s): rounds %d, n_hit %d -> %d, legs at the cap %d, control points per round %s, curve %.2f m (polyline %.2f)"
              % (voxels, fs["rounds"], fs["n_hit_first"], fs["final"]["n_hit"], fs["n_legs_at_cap"], [c for c, _ in stats], tlen, plen))
        print("    fused call (+ read of knots and control points): %s" % t_fused)
        print("    composed loop, %d rounds:                        %s; same spline: %s" % (rounds, t_comp, same))
        if tag == "b" and voxels == 1.0:
            # the serial knot chain of k_bspline_setup at this size: a whole SetParam with the middle points already on the device
            nm = fs["n_cps"] - 6
            mid = api.Trajectory.from_points(ctx, np.zeros((nm, 3), np.float32))
            s2 = api.Bspline(ctx, 3, 3, 2, 2, nm)
            z3 = np.zeros((3, 3), np.float32)
            _, t_set = timed(lambda: s2.set_param(z3, z3, mid, float(nm + 3)))
            print("    wa_bspline_set_param_traj with %d middle points (serial knot chain + constrained points + middle copy): %s" % (nm, t_set))
        b.close()
        samples.close()
    poly.close()
    grid.close()
