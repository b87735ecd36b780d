#!/usr/bin/env python3
"""A fillet weld with a weave, end to end: tool frames at jerk-limited controller ticks (Trajectory.retime_jerk_frames).

The scene is synthetic and self-contained: two plates that meet in a corner (a floor y < m/4 and a wall x < m/4, every z).  The torch
approaches the corner's seam, stops (arc start), lays one pass along z with a triangle weave across the seam, stops (crater fill) and
retreats (both beside the torch's own axis, so every tick has a lateral).  The body of the torch leans out of the corner along
(1, 1, 0), so the lateral -- torch axis x direction of travel -- lies across the seam, between the plates.  Prints one JSON line: the weave, the summaries of the call with the weave, the frames summary of
the same call without it, and how many ticks moved.

    python examples/weave_demo.py [--grid 32] [--jerk 200]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from welding_robot_amd import api  # noqa: E402

WELD = 1   # the tag of the pass and of the two stops at its ends: one run


def corner(m):
    """free[z, y, x] of two plates m / 4 thick, and the unit coordinates of the voxel centres"""
    free = np.ones((m, m, m), np.uint8)
    free[:, :m // 4, :] = 0
    free[:, :, :m // 4] = 0
    c = np.arange(m, dtype=np.float32)
    return free, c


def path(m):
    """approach, stop, pass, stop, retreat: (xyz, dwell per segment, tag per segment); the seam runs along z, 3 voxels off both plates"""
    s = m / 4.0 + 2.5
    far = 0.7 * m
    z0, z1 = 0.2 * m, 0.8 * m
    legs = [np.linspace([far, m / 2.0, z0], [s, s, z0], 6), np.linspace([s, s, z0], [s, s, z1], 13), np.linspace([s, s, z1], [m / 2.0, far, z1], 6)]
    xyz = np.concatenate([legs[0], legs[1], legs[2]]).astype(np.float32)   # (the joints are doubled samples: stops)
    n = len(xyz)
    dwell = np.full(n - 1, -1.0)
    tag = np.zeros(n - 1, np.uint8)
    a, b = len(legs[0]) - 1, len(legs[0]) + len(legs[1]) - 1   # the segments without length at arc start and at crater fill
    dwell[a], dwell[b] = 0.3, 0.5
    tag[a:b + 1] = WELD
    return xyz, dwell, tag


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid", type=int, default=32, help="voxels per edge")
    ap.add_argument("--jerk", type=float, default=200.0, help="jerk limit along the path (sizes the window)")
    ap.add_argument("--pattern", default="triangle", choices=["triangle", "sine", "trapezoid"])
    a = ap.parse_args()
    m = a.grid
    v_max, acc, dec, tick = 6.0, 12.0, 12.0, 0.004
    ctx = api.Context(0)
    free, c = corner(m)
    grid = api.Grid.from_occupancy(ctx, free, c, c, c, 1.0, 0)
    xyz, dwell, tag = path(m)
    traj = api.Trajectory.from_points(ctx, xyz)
    q = np.tile(api.quantise_axes([[1.0, 1.0, 0.0]]), (len(xyz), 1))
    tool = api.torch_tool([0, 16, 32, 48], [1, 1, 2, 2])
    window = api.jerk_window(acc, dec, a.jerk, tick)
    weave = dict(amplitude=0.75, wavelength=1.5, taper=1.0, pattern=api.weave_pattern(a.pattern, 64), tag_mask=0xff, tag_value=WELD)
    kw = dict(dwell=dwell, seg_tag=tag, grid=grid, tool=tool, near_add=2)
    out = traj.retime_jerk_frames(q, v_max, acc, dec, tick, window, weave=weave, **kw)
    plain = traj.retime_jerk_frames(q, v_max, acc, dec, tick, window, **kw)
    moved = int((out[3].points() != plain[3].points()).any(1).sum())
    lat = out[12].points()
    print(json.dumps(dict(grid=m, samples=len(xyz), tick=tick, weave=dict(weave, pattern=a.pattern, P=64), retime=out[6], stops=out[7],
                          jerk=out[8], axes=out[11], frames=out[13], plain=plain[13], moved_ticks=moved,
                          lateral_mid_pass=[round(float(v), 4) for v in lat[len(lat) // 2]])))
    for o in (out, plain):
        for k in (3, 9, 12):
            o[k].close()
    traj.close()
    grid.close()
    ctx.close()


if __name__ == "__main__":
    main()
