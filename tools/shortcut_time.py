#!/usr/bin/env python3
"""Time wa_grid_path_shortcut on the C5-sized batch: the 256^3 synth_grid, 64 weld points, the 2 016 pair paths planned by
examples/plan_batch.py's plan() (150 generations, lazy evaporation).  Prints the batch's size, the median and range of 20 calls
(each a whole call: buffers, copies in and out; HIP events on the context's stream) and what the shortcut does to the paths.
Kernel times: run it alone under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/shortcut_time.py --reps 3`.

    python tools/shortcut_time.py [--reps N] [--max-span N] [--grid N --points P]"""
import ctypes as C
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, span, n, P = arg("--reps", 20), arg("--max-span", 128), arg("--grid", 256), arg("--points", 64)
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
_, paths, _ = pb.plan(ctx, grid, pts, 150, float(24 / 0.35), 7, 0, lazy=True)
batch = [np.asarray(paths[k], np.int64) for k in sorted(paths)]
lens = np.array([len(p) for p in batch])
print("batch: %d paths, %d nodes (mean %.0f, max %d)" % (len(batch), lens.sum(), lens.mean(), lens.max()))

stream = C.c_void_p(ctx.stream)
a, b = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
times = []
for r in range(reps + 1):          # the first call warms up
    ctx.sync()
    hip.hipEventRecord(a, stream)
    wps, lengths = api.shortcut_paths(grid, batch, span)
    hip.hipEventRecord(b, stream)
    hip.hipEventSynchronize(b)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), a, b)
    if r:
        times.append(ms.value)
_, lattice = api.shortcut_paths(grid, batch, 1)
nw = np.array([len(w) for w in wps])
print("wa_grid_path_shortcut max_span %d: median %.3f ms over %d calls (min %.3f, max %.3f)"
      % (span, np.median(times), reps, min(times), max(times)))
print("  waypoints %d of %d nodes; length %.4f of %.4f m (%.3f); every path no longer: %s"
      % (nw.sum(), lens.sum(), lengths.sum(), lattice.sum(), lengths.sum() / lattice.sum(), bool((lengths <= lattice * (1 + 1e-12)).all())))
