#!/usr/bin/env python3
"""Time the tool frames and the weld weave at jerk-limited ticks (wa_traj_retime_jerk_frames) on C5's tour as
tools/jerk_axes_time.py builds it: 256^3 synth_grid, 64 points, --exact-paths --shortcut --fit at 100 001 samples, 1 ms ticks, 64 samples
doubled into stops of 0.5 s, an axis per sample that changes every 97 samples and across every stop.  Every other stretch between two
stops is a weld pass (tag 1, its two stops included) and weaves: a triangle of 64 entries, amplitude one voxel, wavelength four,
taper two.  Whole calls by HIP events on the context's stream, the members ALTERNATING in one process, one warm-up round, then --reps
rounds; median and range per member.  Beside the new call with and without the weave: wa_traj_retime_jerk_axes of this build and,
with --parent-lib, of the parent commit's build (the same launches: it must not move).

    python tools/frames_time.py [--reps N] [--window W] [--K 64] [--parent-lib PATH]"""
import ctypes as C
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import _lib, api, build, synth


def arg(name, default, cast=float):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, W, K = arg("--reps", 5, int), arg("--window", 16, int), arg("--K", 64, int)
LIMITS = (0.25, 1.0, 1.0, 0.5, 0.05, 4.0)
TICK, N_STOPS, DWELL = 0.001, 64, 0.5
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name, flush=True)
ev = [C.c_void_p(), C.c_void_p()]
assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0


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


def close_all(out):
    for v in out if isinstance(out, (tuple, list)) else ():
        if isinstance(v, api.Trajectory):
            v.close()
        else:
            close_all(v)


def alternate(title, members, rounds):
    times, last = {name: [] for name, _, _ in members}, {}
    for r in range(rounds + 1):
        for name, fn, c in members:
            out, ms = once(fn, c)
            last[name] = [v for v in out if not isinstance(v, (api.Trajectory, tuple, list))]
            close_all(out)
            if r:
                times[name].append(ms)
    print(title)
    for name, _, _ in members:
        t = times[name]
        print("    %-52s median %9.3f ms  (min %9.3f, max %9.3f, %d calls)" % (name, np.median(t), min(t), max(t), len(t)), flush=True)
    return last


# ---- C5's tour, 64 of its samples doubled (tools/stops_time.py)
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
stop_seg = at + np.arange(N_STOPS)
m = len(xyz)
dwell = np.full(m - 1, -1.0)
dwell[stop_seg] = DWELL
tool, dirs, _ = pb.torch_tool_and_cone(grid, K)
q = api.quantise_axes(dirs)[((np.arange(m) // 97) + 7 * np.searchsorted(stop_seg, np.arange(m), side="left")) % K]
curve = api.Trajectory.from_points(ctx, xyz)
v_max, acc, dec, a_lat, v_near, near_d2 = LIMITS
kw = dict(dwell=dwell, a_lat=a_lat, v_near=v_near, near_d2=int(near_d2))
print("C5: %d samples (%d doubled), K = %d, tick %g s, %d stops of %g s, W = %d" % (m, N_STOPS, K, TICK, N_STOPS, DWELL, W), flush=True)


tag = (np.searchsorted(stop_seg, np.arange(m - 1), side="left") % 2).astype(np.uint8)   # (a stop carries the tag of the stretch in front of it)
tag[stop_seg[0::2]] = 1                                                                  # ... and a pass owns the stop it begins at too
weave = api.make_weave(1.0 * prec, 4.0 * prec, api.weave_pattern("triangle", 64), taper=2.0 * prec, tag_mask=1, tag_value=1)
fkw = dict(kw, grid=grid, tool=tool, near_add=8, blocked=False, seg_tag=tag, tags=False)
members = [("wa_traj_retime_jerk_axes", lambda: curve.retime_jerk_axes(q, v_max, acc, dec, TICK, W, **fkw), ctx),
           ("wa_traj_retime_jerk_frames, no weave", lambda: curve.retime_jerk_frames(q, v_max, acc, dec, TICK, W, **fkw), ctx),
           ("wa_traj_retime_jerk_frames, weave", lambda: curve.retime_jerk_frames(q, v_max, acc, dec, TICK, W, weave=weave, **fkw), ctx)]
if "--parent-lib" in sys.argv:
    path = sys.argv[sys.argv.index("--parent-lib") + 1]
    held = dict(_lib.SYMBOLS)                                  # the parent's build lacks the new entry point: declare what it has
    probe = C.CDLL(path)
    for name in list(_lib.SYMBOLS):
        if not hasattr(probe, name):
            del _lib.SYMBOLS[name]
    other = api.Context(0, lib_path=path)
    _lib.SYMBOLS.update(held)
    og = api.Grid.from_occupancy(other, free, cx, cy, cz, prec, wall)
    ot = api.Trajectory.from_points(other, xyz)
    members.insert(1, ("wa_traj_retime_jerk_axes, the parent's build",
                       lambda: ot.retime_jerk_axes(q, v_max, acc, dec, TICK, W, **dict(fkw, grid=og)), other))
o = alternate("whole calls, %d samples:" % m, members, reps)
a, b, c = o["wa_traj_retime_jerk_axes"], o["wa_traj_retime_jerk_frames, no weave"], o["wa_traj_retime_jerk_frames, weave"]
eq = lambda x, y: np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
print("    without a weave the outputs wa_traj_retime_jerk_axes has are its bytes:", all(eq(x, y) for x, y in zip(a, b[:len(a)])))
if "--parent-lib" in sys.argv:
    p = o["wa_traj_retime_jerk_axes, the parent's build"]
    print("    wa_traj_retime_jerk_axes gives the parent's bytes:", all(eq(x, y) for x, y in zip(a, p)))
print("    axes, no weave:", b[-2])
print("    axes, weave:   ", c[-2])
print("    frames, no weave:", b[-1])
print("    frames, weave:   ", c[-1], flush=True)
