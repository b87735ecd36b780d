#!/usr/bin/env python3
"""Time the diagonal pose search on the C5-sized job of tools/pose_weighted_time.py: the 256^3 synth_grid, its 64 weld points,
K directions of a cone around +z and the 24-bead torch body of examples/plan_batch.py.  Every time is a whole call (k_reach, buffers,
searches, copies out) between HIP events on the context's stream, after one warm-up call.
  1. like for like: step {1, 2, 3} with zero turn costs against wa_grid_pose_weighted_matrix with hop 1 on the same inputs, the two
     alternating, --reps calls each; the answers must be equal and are compared; the ratio is per level, the level counts being equal,
  2. the 3-4-5 matrix (--reps3 calls), its level count, and one all-pairs wa_grid_pose_diag_paths call beside wa_grid_pose_weighted_paths
     (hop 1): nodes, moves by class, the lattice length and the length after wa_grid_pose_shortcut of both.

    python tools/pose_diag_time.py [--reps N] [--reps3 N] [--grid N --points P] [--dirs K] [--max-turn U] [--rod16 L] [--no-paths] [--only-like]"""
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


reps, reps3, n, P, K, U = arg("--reps", 5), arg("--reps3", 5), arg("--grid", 256), arg("--points", 64), arg("--dirs", 64), arg("--max-turn", 150000)
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
    """nodes, moves by class, lattice length, and the length after wa_grid_pose_shortcut of the reachable pairs' paths"""
    ids = [p for p in ids_all if p is not None]
    ks = [k for k in ks_all if k is not None]
    nx, nxy = grid.nx, grid.nx * grid.ny
    by_class = np.zeros(4, np.int64)
    for p in ids:
        a, b = p[:-1], p[1:]
        by_class += np.bincount((a % nx != b % nx).astype(np.int64) + ((a // nx) % grid.ny != (b // nx) % grid.ny) + (a // nxy != b // nxy), minlength=4)
    lattice = float(api.shortcut_paths(grid, ids, 1)[1].sum())
    short = float(api.pose_shortcut_paths(grid, dirs, tool, U, ids, ks, 128)[3].sum())
    return dict(pairs=len(ids), nodes_total=int(sum(len(p) for p in ids)), moves_by_class=by_class[1:].tolist(), length_total=lattice,
                shortened_length_total=short)


W, nvox = (K + 63) // 64, n ** 3
say("grid %d^3, %d points, K %d (W %d), a %d/16-voxel body, max_turn %d" % (n, P, K, W, length16, U))

# 1. like for like: the diagonals buy nothing at {1, 2, 3}, so the answers and the level counts are those of the weighted search
hop1 = api.pose_costs(1, [], [0])
d123 = api.pose_diag_costs([1, 2, 3], [], [0])
t_old, t_new = [], []
old, _ = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, hop1, pts))            # warm-up of both (the distance field, the code objects)
new, _ = once(lambda: grid.pose_diag_matrix(dirs, tool, U, d123, pts))
for _ in range(reps):                                                                  # alternating: both see the same neighbours on the machine
    old, ms = once(lambda: grid.pose_weighted_matrix(dirs, tool, U, hop1, pts))
    t_old.append(ms)
    new, ms = once(lambda: grid.pose_diag_matrix(dirs, tool, U, d123, pts))
    t_new.append(ms)
same = bool(np.array_equal(old, new))
if reps:                                                                               # (--reps 0: the comparison alone)
    a = line("wa_grid_pose_weighted_matrix, hop 1, no bands, no pen (R = 2), %d points" % P, t_old)
    b = line("wa_grid_pose_diag_matrix, step {1, 2, 3}, no bands, no pen (R = 4), the same points", t_new)
    say("  largest cost %d: about %d levels (weighted) and %d (diagonal); ratio per call %.3f, per level %.3f"
        % (int(old.max()), int(old.max()) + 2, int(new.max()) + 4, b / a, (b / (int(new.max()) + 4)) / (a / (int(old.max()) + 2))))
say("  same answers: %s" % same)
if not same:
    raise SystemExit("the diagonal search with step {1, 2, 3} must return the weighted search's matrix")

if "--only-like" in sys.argv:
    sys.exit(0)

# 2. the 3-4-5 chamfer
d345 = api.pose_diag_costs([3, 4, 5], [], [0])
m3, _ = once(lambda: grid.pose_diag_matrix(dirs, tool, U, d345, pts))
t3 = []
for _ in range(reps3):
    m3, ms = once(lambda: grid.pose_diag_matrix(dirs, tool, U, d345, pts))
    t3.append(ms)
c = line("wa_grid_pose_diag_matrix, step {3, 4, 5}, %d points" % P, t3)
say("  symmetric: %s; unreachable pairs %d (%d by the weighted search); largest cost %d: about %d levels; 3 x the largest hop count %d"
    % (bool(np.array_equal(m3, m3.T)), int((np.triu(m3, 1) < 0).sum()), int((np.triu(old, 1) < 0).sum()), int(m3.max()), int(m3.max()) + 6, 3 * int(old.max())))
if "--no-paths" not in sys.argv:
    ii, jj = np.triu_indices(P, 1)
    (h0, i0, k0), ms0 = once(lambda: grid.pose_weighted_paths(dirs, tool, U, hop1, pts[ii], pts[jj]))
    (h1, i1, k1), ms1 = once(lambda: grid.pose_diag_paths(dirs, tool, U, d345, pts[ii], pts[jj]))
    say("all %d pairs, one call each, no warm-up: wa_grid_pose_weighted_paths (hop 1) %.0f ms, wa_grid_pose_diag_paths (3-4-5) %.0f ms" % (len(ii), ms0, ms1))
    say("  weighted:", totals(i0, k0))
    say("  diagonal:", totals(i1, k1))
