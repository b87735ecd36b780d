#!/usr/bin/env python3
"""Time the clearance entry points with device events on the context's stream, after warm-up:
wa_grid_distance_field at 128^3 and at the 256^3 synth_grid (a fresh grid per call: the field is cached with its grid, so every
timed call builds it from HBM), one wa_grid_inflate and one wa_traj_clearance of a 10^5-sample trajectory.  Prints time and the
achieved bytes/s against the algorithmic bytes (field: 1 + 4 B in the x pass, 4 + 4 in y, 4 + 4 in z = 21 B per voxel).

    python tools/clearance_time.py [--reps N]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth

hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
ctx = api.Context(0)
stream = C.c_void_p(ctx.stream)


def ev():
    e = C.c_void_p()
    assert hip.hipEventCreate(C.byref(e)) == 0
    return e


def timed(fn, setup=None):
    """median device time of fn (ms) between events recorded on the context's stream around it; one warm-up call"""
    a, b = ev(), ev()
    out = []
    for r in range(reps + 1):
        arg = setup() if setup else None
        ctx.sync()
        hip.hipEventRecord(a, stream)
        fn(arg)
        hip.hipEventRecord(b, stream)
        hip.hipEventSynchronize(b)
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), a, b)
        if r:
            out.append(ms.value)
        if arg is not None:
            arg.close()
    return float(np.median(out))


print("device:", ctx.device_name)
for n in (128, 256):
    free, cx, cy, cz, p, wall = synth.synth_grid(n)
    mk = lambda: api.Grid.from_occupancy(ctx, free, cx, cy, cz, p, wall)
    ms = timed(lambda g: ctx.check(ctx.lib.wa_grid_distance_field(g.h, None)), mk)
    byt = 21.0 * n ** 3
    print("distance_field %d^3: %.1f us  %.2f TB/s of algorithmic bytes (%.0f MB)  = %.2f of 8 TB/s"
          % (n, ms * 1e3, byt / (ms * 1e-3) / 1e12, byt / 1e6, byt / (ms * 1e-3) / 8e12))

g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, p, wall)   # 256^3, field built
g.distance_field()
keep = synth.synth_weld_points(free, 256, 64)
ms = timed(lambda _: g.inflate(2.0, keep).close())
print("inflate 256^3 radius 2, 64 keep ids (incl. grid allocation, table upload, n_free recount): %.1f us  (%.2f TB/s of 6 B per voxel)"
      % (ms * 1e3, 6.0 * 256 ** 3 / (ms * 1e-3) / 1e12))
rs = np.random.RandomState(1)
steps = rs.normal(0, 0.7, (100000, 3)).astype(np.float32)
xyz = np.clip(np.cumsum(steps, 0) + 128, 0, 255).astype(np.float32)
t = api.Trajectory.from_points(ctx, xyz)
ms = timed(lambda _: t.clearance(g))
print("clearance of 1e5 samples on 256^3 (incl. buffers and the copies out): %.1f us" % (ms * 1e3))
s = t.clearance(g)[3]
print("  summary:", s)
