#!/usr/bin/env python3
"""Time the weld passes in the timed trajectory (wa_traj_retime_stops, wa_traj_tick_axes_stops, wa_traj_axes_dwells) against the
calls they extend, on C5's tour as tools/ticks_time.py builds it: 256^3 synth_grid, 64 points, --exact-paths --shortcut --fit at 100 001
samples, 1 ms ticks; 64 samples spread evenly over it are doubled, and each doubled sample is a stop of 0.5 s.  Whole calls by HIP
events on the context's stream.  The members of a comparison run in the same process, ALTERNATING, one warm-up round, then --reps
rounds; median and range per member.

    python tools/stops_time.py [--reps N] [--K 64] [--limits V_MAX ACC DEC A_LAT V_NEAR NEAR_D2]
                               [--parent-lib PATH]     (the parent commit's build of the library: its wa_traj_retime and wa_traj_tick_axes
                                                        alternate with this build's on the same samples)"""
import ctypes as C
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import _lib, api, build, synth


def arg(name, default, n=1, cast=float):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name) + 1
    return cast(sys.argv[i]) if n == 1 else tuple(cast(v) for v in sys.argv[i:i + n])


reps = arg("--reps", 8, cast=int)
K = arg("--K", 64, cast=int)
LIMITS = arg("--limits", (0.25, 1.0, 1.0, 0.5, 0.05, 4.0), 6)
TICK, N_STOPS, DWELL = 0.001, 64, 0.5
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
ev = [C.c_void_p(), C.c_void_p()]
assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0
Q = 1 << 30


def once(fn, c):
    stream = C.c_void_p(c.stream)
    c.sync()
    hip.hipEventRecord(ev[0], stream)
    out = fn()
    hip.hipEventRecord(ev[1], stream)
    hip.hipEventSynchronize(ev[1])
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
    return out, ms.value


def alternate(title, members):
    """members: (name, fn, context).  One round calls every member once, in order; the first round warms up."""
    times, outs = {name: [] for name, _, _ in members}, {}
    for r in range(reps + 1):
        for name, fn, c in members:
            outs[name], ms = once(fn, c)
            if r:
                times[name].append(ms)
    print(title)
    for name, _, _ in members:
        t = times[name]
        print("    %-58s median %8.3f ms  (min %8.3f, max %8.3f, %d calls)" % (name, np.median(t), min(t), max(t), len(t)))
    return outs


def close_all(outs, k):
    for o in outs.values():
        if o[k] is not None:
            o[k].close()


# ---- C5's tour, 64 of its samples doubled
n, P, n_samples = 256, 64, 100001
free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
pts = synth.synth_weld_points(free, n, P, seed=7)
cost, paths, _ = pb.plan_exact(grid, pts, shortcut=128)
short = pb.plan.last_shortcut
edges = api.gtsp_solve(ctx, cost, mode=api.RNG_DEV, seed=7)["edges"][0][:-1]
rev = [1 if a > b else 0 for a, b in edges]
wsegs = [short[(min(a, b), max(a, b))] for a, b in edges]
poly = api.Trajectory.stitch(grid, wsegs, rev)
_, samples, _, _ = poly.fit(grid, 3, None, 6, n_samples)
base = samples.points()
at = (np.arange(1, N_STOPS + 1) * (n_samples // (N_STOPS + 1))).astype(np.int64)
xyz = np.insert(base, at, base[at], axis=0)
stop_seg = at + np.arange(N_STOPS)                             # the doubled sample k sits at at[k] + k and at[k] + k + 1
assert np.array_equal(xyz[stop_seg], xyz[stop_seg + 1])
m = len(xyz)
dwell = np.full(m - 1, -1.0)
dwell[stop_seg] = DWELL
tool, dirs, _ = pb.torch_tool_and_cone(grid, K)
# an axis per sample that changes every 97 samples and across every stop
q = api.quantise_axes(dirs)[((np.arange(m) // 97) + 7 * np.searchsorted(stop_seg, np.arange(m), side="left")) % K]
tags = np.zeros(m - 1, np.uint8)
tags[stop_seg[0]:stop_seg[-1]] = 1
curve = api.Trajectory.from_points(ctx, xyz)
v_max, acc, dec, a_lat, v_near, near_d2 = LIMITS
kw = dict(a_lat=a_lat, grid=grid, v_near=v_near, near_d2=int(near_d2))
print("C5: %d samples (%d doubled), K = %d, tick %g s, %d stops of %g s" % (m, N_STOPS, K, TICK, N_STOPS, DWELL))

other = None
if "--parent-lib" in sys.argv:
    path = sys.argv[sys.argv.index("--parent-lib") + 1]
    held = dict(_lib.SYMBOLS)                                  # the parent's build lacks the new entry points: declare what it has
    probe = C.CDLL(path)
    for name in list(_lib.SYMBOLS):
        if not hasattr(probe, name):
            del _lib.SYMBOLS[name]
    other = api.Context(0, lib_path=path)
    _lib.SYMBOLS.update(held)
    og = api.Grid.from_occupancy(other, free, cx, cy, cz, prec, wall)
    ot = api.Trajectory.from_points(other, xyz)

# ---- pair 1: the timing
members = [("wa_traj_retime", lambda: curve.retime(v_max, acc, dec, TICK, **kw), ctx),
           ("wa_traj_retime_stops, dwell = NULL", lambda: curve.retime_stops(v_max, acc, dec, TICK, dwell=None, **kw), ctx),
           ("wa_traj_retime_stops, no entry >= 0 (the stops kernels)", lambda: curve.retime_stops(v_max, acc, dec, TICK, dwell=np.full(m - 1, -1.0), **kw), ctx),
           ("wa_traj_retime_stops, %d stops of %g s" % (N_STOPS, DWELL), lambda: curve.retime_stops(v_max, acc, dec, TICK, dwell=dwell, **kw), ctx)]
if other is not None:
    members.insert(1, ("wa_traj_retime, the parent's build", lambda: ot.retime(v_max, acc, dec, TICK, **dict(kw, grid=og)), other))
o = alternate("the timing, %d samples:" % m, members)
plain, stopped = o["wa_traj_retime"], o[members[-1][0]]
for name in o:
    if name != members[-1][0]:
        same = all(np.array_equal(a, b) for a, b in zip(o[name][:3], plain[:3])) and o[name][3].points().tobytes() == plain[3].points().tobytes()
        print("    %s: same bytes as wa_traj_retime: %s" % (name, same))
print("    without stops: %.3f s, %d ticks; with: %.3f s, %d ticks; %s" %
      (plain[4]["time_q"] / Q, plain[4]["n_ticks"], stopped[4]["time_q"] / Q, stopped[4]["n_ticks"], stopped[5]))
close_all(o, 3)

# ---- pair 2: the tick axes, on the result WITHOUT dwells and on the one with
time_q, w_q = plain[0], plain[1]
tq2, wq2 = stopped[0], stopped[1]
members = [("wa_traj_tick_axes", lambda: curve.tick_axes(q, time_q, w_q, acc, dec, TICK, grid, tool, near_add=8), ctx),
           ("wa_traj_tick_axes_stops, no dwell, no tags", lambda: curve.tick_axes_stops(q, time_q, w_q, acc, dec, TICK, grid=grid, tool=tool, near_add=8), ctx),
           ("wa_traj_tick_axes_stops, no dwell, tags", lambda: curve.tick_axes_stops(q, time_q, w_q, acc, dec, TICK, seg_tag=tags, grid=grid, tool=tool, near_add=8), ctx),
           ("wa_traj_tick_axes_stops, %d dwells, tags" % N_STOPS, lambda: curve.tick_axes_stops(q, tq2, wq2, acc, dec, TICK, seg_tag=tags, grid=grid, tool=tool, near_add=8), ctx)]
if other is not None:
    members.insert(1, ("wa_traj_tick_axes, the parent's build", lambda: ot.tick_axes(q, time_q, w_q, acc, dec, TICK, og, tool, near_add=8), other))
o = alternate("the tick axes:", members)
ref = o["wa_traj_tick_axes"]
for name in list(o)[1:-1]:
    same = o[name][0].points().tobytes() == ref[0].points().tobytes() and np.array_equal(o[name][1], ref[1]) and o[name][2] == ref[2]
    print("    %s: same bytes as wa_traj_tick_axes: %s" % (name, same))
last = o[members[-1][0]]
print("    with dwells: %s\n    %s" % (last[2], last[4]))
close_all(o, 0)

# ---- the dwells a turn rate asks for
o = alternate("the dwells:", [("wa_traj_axes_dwells (omega = 2)", lambda: curve.axis_dwells(q, 2.0, dwell), ctx)])
print("    %s" % (o["wa_traj_axes_dwells (omega = 2)"][1],))
