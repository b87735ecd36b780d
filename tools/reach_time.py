#!/usr/bin/env python3
"""Time the torch-fit planning grids (wa_grid_tool_reach, wa_grid_tool_fit) on C5's synthetic 256^3 grid with the tool and cone of
profiles/torch/README.md (K = 64 directions, 24 beads over 0.3 voxels) and, because that tool is shorter than a voxel, with a 12-voxel
rod of 24 beads as well.  Whole calls by HIP events on the context's stream (one warm-up, then median and range).  Counted from the
restatement's rule, not timed: the share of free voxels the far-voxel shortcut skips (free voxels with d2 >= R^2).

The yardstick is the code that existed before: the voxel centres of the same grid in raster order through k_torch_nodes, that is
Trajectory.torch_axes(..., feas=True) with one leg per z slab, in chunks of --slabs slabs; its feasibility bytes are held against the
counts (same blocked pairs).

Kernel times and bead loads per second: run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python
tools/reach_time.py --reps 3` and divide the loads printed here by the kernel time of k_reach; --no-prune-lib PATH runs the same on a
library built with -DWA_REACH_NO_PRUNE (python -m welding_robot_amd.build -DWA_REACH_NO_PRUNE --out=PATH), the shortcut compiled out.

    python tools/reach_time.py [--grid N] [--reps N] [--slabs N] [--no-yardstick] [--no-prune-lib PATH]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n, reps, slabs = arg("--grid", 256), arg("--reps", 10), arg("--slabs", 32)
lib_path = arg("--no-prune-lib", "") or None
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0, lib_path=lib_path)
print("device:", ctx.device_name, "| library:", lib_path or "the product", "| grid %d^3" % n)
stream = C.c_void_p(ctx.stream)
ev = [C.c_void_p(), C.c_void_p()]
assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0


def timed(fn, k=reps):
    out, times = None, []
    for r in range(k + 1):          # the first call warms up
        ctx.sync()
        hip.hipEventRecord(ev[0], stream)
        out = fn()
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        if r:
            times.append(ms.value)
    return out, float(np.median(times)), "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(times), min(times), max(times), k)


def prune_radius(dist16, r2):
    return max((int(d) + 15) // 16 + 2 + int(np.floor(np.sqrt(int(r)))) + 1 for d, r in zip(dist16, r2))


free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
d2 = grid.distance_field()
pts = synth.synth_weld_points(free, n, 64, seed=7)
K = 64
dirs = api.torch_cone(K, 1.2)
length16 = int(min(65536, round(16 * 0.3 / float(grid.precision))))
tools = [("profile tool, 24 beads over %.2f voxels" % (length16 / 16), np.rint(np.linspace(0, length16, 24)).astype(np.int64)),
         ("rod, 24 beads over 12 voxels", np.rint(np.linspace(0, 192, 24)).astype(np.int64))]
for name, dist16 in tools:
    r2 = np.full(24, 1, np.int64)
    tool = api.torch_tool(dist16, r2)
    R = prune_radius(dist16, r2)
    far = int(((free != 0) & (d2.astype(np.int64) >= R * R)).sum())
    print("%s, K = %d: R = %d, the shortcut skips %d of %d free voxels (%.2f %%)" % (name, K, R, far, grid.n_free, 100.0 * far / grid.n_free))
    (_, count, s), ms, text = timed(lambda: grid.torch_reach(dirs, tool, masks=False))
    pairs = grid.n * K
    print("    wa_grid_tool_reach (counts only): %s = %.3f ns per (voxel, direction) pair of all %d" % (text, ms * 1e6 / pairs, pairs))
    print("        summary %s" % s)
    print("        bead loads if no direction left its bead loop early: %d per call (free voxels x K x 24; the kernel leaves a "
          "direction once no lane of the wavefront is alive, so it issues fewer)" % (grid.n_free * K * 24))
    f, ms_fit, text = timed(lambda: grid.torch_fit(dirs, tool, 1, pts, 16))
    print("    wa_grid_tool_fit (min_dirs 1, 64 keep ids, keep_r2 16): %s; free voxels %d -> %d" % (text, grid.n_free, f.n_free))
    f.close()
    if "--no-yardstick" in sys.argv or lib_path:
        continue
    # the yardstick: the same voxels as samples of a trajectory, one leg per slab
    total_ms, blocked = 0.0, 0
    zz, yy, xx = np.meshgrid(cz[:slabs], cy, cx, indexing="ij")
    base = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1).astype(np.float32)
    for z0 in range(0, n, slabs):
        nz = min(slabs, n - z0)
        xyz = base[:nz * n * n].copy()
        xyz[:, 2] = np.repeat(cz[z0:z0 + nz], n * n)
        t = api.Trajectory.from_points(ctx, xyz)
        off = np.arange(nz + 1, dtype=np.int64) * n * n
        r, ms, _ = timed(lambda: t.torch_axes(grid, dirs, tool, off=off, feas=True), 1)
        total_ms += ms
        sl = slice(z0 * n * n, (z0 + nz) * n * n)
        fr = free[sl] != 0
        assert np.array_equal((r["feas"] != 255).sum(1)[fr], count[sl][fr]), "the trajectory planner and the grid kernel disagree"
        blocked += r["summary"]["n_blocked_pairs"]
        t.close()
    print("    yardstick, Trajectory.torch_axes(feas=True) over every voxel centre in %d chunks of %d slabs: %.1f ms in all = %.3f ns per pair "
          "(its calls also run k_torch_dp and copy the n x K table back; the kernel-only figure is k_torch_nodes in the kernel trace)"
          % ((n + slabs - 1) // slabs, slabs, total_ms, total_ms * 1e6 / pairs))
