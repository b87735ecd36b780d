#!/usr/bin/env python3
"""Time wa_grid_pose_shortcut on the C5-sized batch beside wa_grid_path_shortcut on the same paths: the 256^3 synth_grid, 64 weld
points, the 2 016 hop-optimal pair paths of wa_grid_geodesic_paths, K = 64 directions and the 24-bead torch of examples/plan_batch.py.
Every node gets the lowest open direction of its voxel (0 where none is open), so that the timing needs no pose search.  Prints the
batch's size, the median and range of the calls (each a whole call: the masks, buffers, copies in and out; HIP events on the
context's stream) and the hold counts.  Kernel times: run it alone under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/pose_shortcut_time.py --reps 3`.

    python tools/pose_shortcut_time.py [--reps N] [--max-span N] [--max-turn U] [--grid N --points P --dirs K]"""
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


reps, span, n, P, K, max_turn = arg("--reps", 20), arg("--max-span", 128), arg("--grid", 256), arg("--points", 64), arg("--dirs", 64), arg("--max-turn", -1)
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
ids = np.asarray(pts, np.int64)
pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
hops, paths = api.geodesic_paths(grid, [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs])
batch = [np.asarray(p, np.int64) for p in paths if p is not None]
lens = np.array([len(p) for p in batch])
print("batch: %d paths, %d nodes (mean %.0f, max %d)" % (len(batch), lens.sum(), lens.mean(), lens.max()))
tool, dirs, _ = pb.torch_tool_and_cone(grid, K)
mask, count, reach = grid.torch_reach(dirs, tool)
print("reach:", reach)


def lowest_open(p):
    """per node the lowest open direction of its voxel, 0 where none is open"""
    k = np.zeros(len(p), np.int32)
    todo = np.ones(len(p), bool)
    for w in range(mask.shape[0]):
        m = mask[w, p]
        low = m & (~m + np.uint64(1))                       # the lowest set bit
        hit = todo & (m != 0)
        k[hit] = w * 64 + np.log2(low[hit].astype(np.float64)).astype(np.int32)
        todo &= ~hit
    return k


kss = [lowest_open(p) for p in batch]
del mask

stream = C.c_void_p(ctx.stream)
a, b = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0


def timed(call):
    times, res = [], None
    for r in range(reps + 1):          # the first call warms up
        ctx.sync()
        hip.hipEventRecord(a, stream)
        res = call()
        hip.hipEventRecord(b, stream)
        hip.hipEventSynchronize(b)
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), a, b)
        if r:
            times.append(ms.value)
    return times, res


t_plain, (wps, plain) = timed(lambda: api.shortcut_paths(grid, batch, span))
t_reach, _ = timed(lambda: grid.torch_reach(dirs, tool, masks=False))
t_pose, (pw, pk, holds, lengths, summary) = timed(lambda: api.pose_shortcut_paths(grid, dirs, tool, max_turn, batch, kss, span))
for name, t in (("wa_grid_path_shortcut", t_plain), ("wa_grid_tool_reach (counts only, no masks)", t_reach), ("wa_grid_pose_shortcut", t_pose)):
    print("%s max_span %d: median %.3f ms over %d calls (min %.3f, max %.3f)" % (name, span, np.median(t), reps, min(t), max(t)))
_, lattice = api.shortcut_paths(grid, batch, 1)
print("  plain: waypoints %d of %d nodes; length %.4f of %.4f m" % (sum(len(w) for w in wps), lens.sum(), plain.sum(), lattice.sum()))
print("  pose:  waypoints %d; length %.4f m; paths shorter than their plain shortcut (the greedy rule promises no order): %d"
      % (summary["n_waypoints"], lengths.sum(), int((lengths < plain).sum())))
print("  summary:", summary)
