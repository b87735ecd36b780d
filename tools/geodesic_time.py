#!/usr/bin/env python3
"""Time the exact shortest-path fields on the C5-sized job: the 256^3 synth_grid and its 64 weld points.  Prints, for the hop matrix
(wa_grid_geodesic_matrix), the stored fields (wa_grid_geodesic_fields) and the paths of all 2 016 pairs (wa_grid_geodesic_paths, the
second of api.geodesic_paths' two calls), the median and range of --reps calls after a warm-up (each a whole call: buffers, searches,
copies out; HIP events on the context's stream), the number of levels (the largest hop count of a field + 1 launches look at a frontier)
and the traffic model of a level.  Kernel times: run it alone under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/geodesic_time.py --reps 3`.

    python tools/geodesic_time.py [--reps N] [--grid N --points P] [--no-fields]"""
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
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
stream = C.c_void_p(ctx.stream)
a, b = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0


def timed(fn, reps):
    times, out = [], None
    for r in range(reps + 1):          # the first call warms up (and builds the bit-packed occupancy)
        ctx.sync()
        hip.hipEventRecord(a, stream)
        out = fn()
        hip.hipEventRecord(b, stream)
        hip.hipEventSynchronize(b)
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), a, b)
        if r:
            times.append(ms.value)
    return out, times


def line(name, times):
    print("%s: median %.3f ms over %d calls (min %.3f, max %.3f)" % (name, np.median(times), len(times), min(times), max(times)))


m, t = timed(lambda: grid.geodesic_matrix(pts), reps)
line("wa_grid_geodesic_matrix %d points on %d^3" % (P, n), t)
print("  largest hop count between two points %d (a search stops when its row is full); symmetric %s, unreachable pairs %d"
      % (m.max(), bool(np.array_equal(m, m.T)), int((np.triu(m, 1) < 0).sum())))
W = (n + 63) // 64
words = W * n * n
print("  traffic model of one level, per live source: read frontier + visited + free words, write frontier (+ visited where new): "
      "%.2f MB of bitmap words (%d words of 8 bytes each way); %d sources keep %.0f MB of bitmaps"
      % (4 * words * 8 / 1e6, words, P, 3 * P * words * 8 / 1e6))
if "--no-fields" not in sys.argv:
    f, t = timed(lambda: grid.geodesic_fields(pts), max(3, reps // 4))
    line("wa_grid_geodesic_fields %d sources (fields copied to the host: %.0f MB)" % (P, f.nbytes / 1e6), t)
    print("  levels per source: min %d, max %d; same numbers as the matrix: %s" % (f.max(1).min(), f.max(1).max(), bool(np.array_equal(f[:, pts], m))))
    del f
    ii, jj = np.triu_indices(P, 1)
    (hops, paths), t = timed(lambda: api.geodesic_paths(grid, pts[ii], pts[jj]), max(3, reps // 4))
    line("api.geodesic_paths %d pairs (two calls: hops, then paths)" % len(ii), t)
    print("  path nodes %d (mean %.0f, max %d); hops equal the matrix: %s"
          % (sum(len(p) for p in paths), np.mean([len(p) for p in paths]), max(len(p) for p in paths), bool(np.array_equal(hops, m[ii, jj]))))
