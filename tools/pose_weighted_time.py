#!/usr/bin/env python3
"""Time the turn-cost pose search on the C5-sized job of tools/pose_time.py: the 256^3 synth_grid, its 64 weld points, K
directions of a cone around +z and the 24-bead torch body of examples/plan_batch.py.  Every time is a whole call (k_reach, buffers,
searches, copies out) between HIP events on the context's stream, after one warm-up call.
  1. the zero-cost description (hop 1, no bands, no pen: R = 2) against wa_grid_pose_matrix on the same inputs, the two alternating,
     --reps calls each; the bytes are compared,
  2. a three-band description with penalties from wa_grid_clearance_costs (R = 12): the matrix (--reps3 calls), the level count, the
     traffic model of a level, and one all-pairs wa_grid_pose_weighted_paths call beside wa_grid_pose_paths with the totals of hops,
     direction changes and U.

    python tools/pose_weighted_time.py [--reps N] [--reps3 N] [--grid N --points P] [--dirs K] [--max-turn U] [--rod16 L] [--no-paths] [--only-zero]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def say(*a):
    print(*a, flush=True)


reps, reps3, n, P, K, U = arg("--reps", 5), arg("--reps3", 2), arg("--grid", 256), arg("--points", 64), arg("--dirs", 64), arg("--max-turn", 150000)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
say("device:", ctx.device_name)
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
length16 = arg("--rod16", int(min(65536, round(16 * 0.3 / float(grid.precision)))))          # default: the 300 mm body of examples/plan_batch.py
tool = api.torch_tool(np.rint(np.linspace(0, length16, 24)).astype(np.int64), np.full(24, 1))
dirs = api.torch_cone(K, 1.2)
stream = C.c_void_p(ctx.stream)
ea, eb = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(ea)) == 0 and hip.hipEventCreate(C.byref(eb)) == 0


def once(fn):
    ctx.sync()
    hip.hipEventRecord(ea, stream)
    out = fn()
    hip.hipEventRecord(eb, stream)
    hip.hipEventSynchronize(eb)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), ea, eb)
    return out, ms.value


def line(name, times):
    say("%s: median %.3f ms over %d calls (min %.3f, max %.3f)" % (name, np.median(times), len(times), min(times), max(times)))
    return float(np.median(times))


def totals(ids_all, ks_all):
    q = api.quantise_axes(dirs).astype(np.int64)
    hops = changes = turn = 0
    for ids, ks in zip(ids_all, ks_all):
        if ks is None or len(ks) < 2:
            continue
        d = q[ks[:-1]] - q[ks[1:]]
        hops, changes, turn = hops + len(ids) - 1, changes + int((ks[:-1] != ks[1:]).sum()), turn + int(((d * d).sum(1) >> 10).sum())
    return hops, changes, turn


W, nvox = (K + 63) // 64, n ** 3
say("grid %d^3, %d points, K %d (W %d), a %d/16-voxel body, max_turn %d" % (n, P, K, W, length16, U))

# 1. the smallest ring against the hop search
zero = api.pose_costs(1, [], [0])
t_old, t_new = [], []
old, _ = once(lambda: grid.pose_matrix(dirs, tool, U, pts))            # warm-up of both (the distance field, the code objects)
new, _ = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, zero, pts))
for _ in range(reps):                                                   # alternating: both see the same neighbours on the machine
    old, ms = once(lambda: grid.pose_matrix(dirs, tool, U, pts))
    t_old.append(ms)
    new, ms = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, zero, pts))
    t_new.append(ms)
a = line("wa_grid_pose_matrix, %d points" % P, t_old)
b = line("wa_grid_pose_weighted_matrix, hop 1, no bands, no pen (R = 2), the same points", t_new)
say("  same bytes: %s; largest hop count %d; ratio weighted / hops %.3f" % (bool(np.array_equal(old, new)), int(old.max()), b / a))

if "--only-zero" in sys.argv:
    sys.exit(0)

# 2. three bands and clearance penalties
pen = np.clip(grid.clearance_costs([1, 4]).astype(np.int32) - 1, 0, 15).astype(np.uint8)
bands, tcs = [5000, 30000, 80000], [0, 2, 4, 7]
costs = api.pose_costs(2, bands, tcs, pen)
R = 2 + tcs[-1] + int(pen[free.ravel() != 0].max()) + 1
n_w = len(set(tcs))
say("three bands %s, turn costs %s, hop 2, pen = clearance_costs([1, 4]) - 1 (largest %d): R = %d; per source %.0f MB of ring and seen"
    % (bands, tcs, int(pen[free.ravel() != 0].max()), R, (R + 1) * W * 8 * nvox / 1e6))
m3, _ = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, costs, pts))
t3 = []
for _ in range(reps3):
    m3, ms = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, costs, pts))
    t3.append(ms)
c = line("wa_grid_pose_weighted_matrix, three bands, %d points" % P, t3)
levels = int(m3.max()) + R
adj = m3 - pen[pts][None, :].astype(np.int32)
say("  d(i, j) - pen[j] symmetric: %s; unreachable pairs %d (%d by hops); largest cost %d: about %d levels"
    % (bool(np.array_equal(np.where(m3 >= 0, adj, -1), np.where(m3.T >= 0, adj.T, -1))), int((np.triu(m3, 1) < 0).sum()),
       int((np.triu(old, 1) < 0).sum()), int(m3.max()), levels))
per_level = (3 + n_w) * W * 8 * nvox + nvox
say("  traffic model of one level, per live source: open + seen + the slot written + %d gathered sets + pen = %.0f MB; %d levels x %d "
    "sources = %.1f TB in %.3f s = %.0f GB/s averaged over the call (an upper bound on the traffic: lanes without a candidate gather nothing, "
    "sources whose row is full stop early)" % (n_w, per_level / 1e6, levels, P, levels * P * per_level / 1e12, c / 1e3, levels * P * per_level / 1e9 / (c / 1e3)))
if "--no-paths" not in sys.argv:
    ii, jj = np.triu_indices(P, 1)
    (h0, i0, k0), ms0 = once(lambda: grid.pose_paths(dirs, tool, U, pts[ii], pts[jj]))
    (h1, i1, k1), ms1 = once(lambda: grid.pose_weighted_paths(dirs, tool, U, costs, pts[ii], pts[jj]))
    say("all %d pairs, one call each, no warm-up: wa_grid_pose_paths %.0f ms, wa_grid_pose_weighted_paths %.0f ms" % (len(ii), ms0, ms1))
    say("  reachable pairs %d / %d; hops, direction changes, sum of U: pose_paths %s, weighted %s"
        % (int((h0 >= 0).sum()), int((h1 >= 0).sum()), totals(i0, k0), totals(i1, k1)))
