#!/usr/bin/env python3
"""Time the clearance-weighted shortest paths on the C5-sized job: the 256^3 synth_grid and its 64 weld points.  Prints the median and
range of --reps whole calls after a warm-up (buffers, cost upload and packing, searches, copies out; HIP events on the context's stream)
for: wa_grid_geodesic_matrix and wa_grid_weighted_matrix with all-ones costs, alternating in one run (the same work, old kernel against
new); wa_grid_clearance_costs; the matrix and the paths of all 2 016 pairs with bands 1, 4, 9 (or --bands R: 1^2 .. R^2); and for each
the levels a search runs (the largest distance + 1 launches see a frontier) and the traffic model of a level.  Kernel times (mean and
longest level): run it alone under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/weighted_time.py --reps 3`.

    python tools/weighted_time.py [--reps N] [--grid N --points P] [--bands R] [--no-paths]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, n, P, R = arg("--reps", 20), arg("--grid", 256), arg("--points", 64), arg("--bands", 3)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
stream = C.c_void_p(ctx.stream)
a, b = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0


def once(fn):
    ctx.sync()
    hip.hipEventRecord(a, stream)
    out = fn()
    hip.hipEventRecord(b, stream)
    hip.hipEventSynchronize(b)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), a, b)
    return out, ms.value


def timed(fns, reps):
    """the calls of fns in turn, reps + 1 rounds; the first round warms up (and builds the bit-packed occupancy / the distance field)"""
    times, outs = [[] for _ in fns], [None] * len(fns)
    for r in range(reps + 1):
        for k, fn in enumerate(fns):
            outs[k], ms = once(fn)
            if r:
                times[k].append(ms)
    return outs, times


def line(name, times):
    print("%s: median %.3f ms over %d calls (min %.3f, max %.3f)" % (name, np.median(times), len(times), min(times), max(times)))


words = ((n + 63) // 64) * n * n
ones = np.ones(grid.n, np.uint8)
(m0, m1), (t0, t1) = timed([lambda: grid.geodesic_matrix(pts), lambda: grid.weighted_matrix(ones, pts)], reps)
line("wa_grid_geodesic_matrix %d points on %d^3" % (P, n), t0)
line("wa_grid_weighted_matrix, all-ones costs (uploads and packs %.0f MB of cost bytes per call)" % (grid.n / 1e6), t1)
print("  same numbers: %s; largest distance %d: the longest search runs that many levels + 1; per level and live source the old kernel moves"
      " frontier + visited + free in, frontier out (%.2f MB of bitmap words), the new one frontier + touched + free in, one ring slot out"
      " (the same), and the cost planes (3 words) only where a word has newly touched voxels" % (bool(np.array_equal(m0, m1)), m0.max(), 4 * words * 8 / 1e6))
bands = [k * k for k in range(1, R + 1)]
(cost,), (t,) = timed([lambda: grid.clearance_costs(bands)], reps)
line("wa_grid_clearance_costs bands %s (distance field kept from the warm-up; %.0f MB copied to the host)" % (bands, grid.n / 1e6), t)
print("  voxels per cost:", {int(c): int(k) for c, k in zip(*np.unique(cost, return_counts=True))})
Wm = int(cost.max())
(m,), (t,) = timed([lambda: grid.weighted_matrix(cost, pts)], reps)
line("wa_grid_weighted_matrix bands %s (W = %d: %d bitmaps per source, %.0f MB for %d sources)" % (bands, Wm, Wm + 2, (Wm + 2) * P * words * 8 / 1e6, P), t)
c = cost[pts].astype(np.int64)
print("  largest distance %d (hops: %d); unreachable pairs %d; dist(i, j) - dist(j, i) = cost[j] - cost[i] everywhere: %s"
      % (m.max(), m0.max(), int((m < 0).sum()), bool(np.array_equal(m - m.T, c[None, :] - c[:, None]))))
if "--no-paths" not in sys.argv:
    ii, jj = np.triu_indices(P, 1)
    ((dist, lens, paths),), (t,) = timed([lambda: api.weighted_paths(grid, cost, pts[ii], pts[jj])], max(3, reps // 4))
    line("api.weighted_paths %d pairs (two calls: distances and node counts, then paths; a field of %.0f MB per start)" % (len(ii), grid.n * 4 / 1e6), t)
    print("  path nodes %d (mean %.0f, max %d), steps over the hop optimum %d; distances equal the matrix: %s"
          % (int(lens.sum()), lens.mean(), lens.max(), int((lens - 1 - m0[ii, jj]).sum()), bool(np.array_equal(dist, m[ii, jj]))))
