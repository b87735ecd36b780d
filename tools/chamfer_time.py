#!/usr/bin/env python3
"""Time the 26-neighbour chamfer fields on the C5-sized job: the 256^3 synth_grid and its 64 weld points.  Prints the median and range of
--reps whole calls after a warm-up (buffers, searches, copies out; HIP events on the context's stream) for: wa_grid_geodesic_matrix and
wa_grid_chamfer_matrix with step {1, 2, 3}, alternating in one run (the same answers and the same number of productive levels: hop
kernel against pull kernel); the matrix and the paths of all 2 016 pairs with --step (default 3 4 5); and for each the levels a search
runs and the traffic model of a level.  Kernel times (mean and longest level): run it alone under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/chamfer_time.py --reps 3`.

    python tools/chamfer_time.py [--reps N] [--grid N --points P] [--step A B C] [--no-paths]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, n, P = arg("--reps", 20), arg("--grid", 256), arg("--points", 64)
step = [int(v) for v in sys.argv[sys.argv.index("--step") + 1:sys.argv.index("--step") + 4]] if "--step" in sys.argv else [3, 4, 5]
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
    """the calls of fns in turn, reps + 1 rounds; the first round warms up (and builds the bit-packed occupancy)"""
    times, outs = [[] for _ in fns], [None] * len(fns)
    for r in range(reps + 1):
        for k, fn in enumerate(fns):
            outs[k], ms = once(fn)
            if r:
                times[k].append(ms)
    return outs, times


def line(name, times):
    print("%s: median %.3f ms over %d calls (min %.3f, max %.3f)" % (name, np.median(times), len(times), min(times), max(times)))
    return float(np.median(times))


words = ((n + 63) // 64) * n * n
(m0, m1), (t0, t1) = timed([lambda: grid.geodesic_matrix(pts), lambda: grid.chamfer_matrix((1, 2, 3), pts)], reps)
g_ms = line("wa_grid_geodesic_matrix %d points on %d^3" % (P, n), t0)
c_ms = line("wa_grid_chamfer_matrix, step {1, 2, 3}", t1)
levels = int(m0.max()) + 1
print("  same numbers: %s; largest distance %d: the longest search runs that many levels + 1; whole-call ratio %.2f.  Per level and live source"
      " the hop kernel moves frontier + visited + free in, frontier out (%.2f MB of bitmap words); the pull kernel up to three history"
      " slots + done + free in, one slot out (%.2f MB), its neighbour rows and the other sources' free words out of the caches"
      % (bool(np.array_equal(m0, m1)), m0.max(), c_ms / g_ms, 4 * words * 8 / 1e6, 6 * words * 8 / 1e6))
print("  per level (whole call / levels of the longest search): hop %.1f us, pull %.1f us" % (1e3 * g_ms / levels, 1e3 * c_ms / levels))
M = max(step)
(m,), (t,) = timed([lambda: grid.chamfer_matrix(step, pts)], reps)
ms = line("wa_grid_chamfer_matrix step %s (R = %d: %d bitmaps per source, %.0f MB for %d sources)" % (step, M + 1, M + 2, (M + 2) * P * words * 8 / 1e6, P), t)
print("  largest distance %d (hops: %d) = launches of the longest search - 1: %.1f us per level; unreachable pairs %d; symmetric: %s; "
      "dist <= %d * hops everywhere: %s" % (m.max(), m0.max(), 1e3 * ms / (int(m.max()) + 1), int((m < 0).sum()), bool(np.array_equal(m, m.T)),
                                            step[0], bool((m <= step[0] * m0).all())))
if "--no-paths" not in sys.argv:
    ii, jj = np.triu_indices(P, 1)
    ((dist, lens, paths),), (t,) = timed([lambda: api.chamfer_paths(grid, step, pts[ii], pts[jj])], max(3, reps // 4))
    line("api.chamfer_paths %d pairs (two calls: distances and node counts, then paths; a field of %.0f MB per start)" % (len(ii), grid.n * 4 / 1e6), t)
    print("  path nodes %d (mean %.0f, max %d), hop-optimal paths have %d; distances equal the matrix: %s"
          % (int(lens.sum()), lens.mean(), lens.max(), int((m0[ii, jj] + 1).sum()), bool(np.array_equal(dist, m[ii, jj]))))
