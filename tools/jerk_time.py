#!/usr/bin/env python3
"""Time the jerk-limited controller ticks (wa_traj_retime_jerk) on C5's tour as tools/stops_time.py builds it: 256^3
synth_grid, 64 points, --exact-paths --shortcut --fit at 100 001 samples, 1 ms ticks, 64 samples doubled into stops of 0.5 s.  Whole
calls by HIP events on the context's stream, the members ALTERNATING in one process, one warm-up round, then --reps rounds; median and
range per member.  The yardsticks: wa_traj_retime_stops on the same input (the unfiltered cost), and with --composed the same filter
composed from what exists -- wa_traj_retime_stops, the read-back, tests/jerk_ref.py's arcs, window means and positions in numpy,
wa_traj_from_points (once, for one window: it takes the host a while; it lowers no cap, so its profile is the unfiltered one).

    python tools/jerk_time.py [--reps N] [--windows 1 16 128] [--limits V_MAX ACC DEC A_LAT V_NEAR NEAR_D2] [--composed W]"""
import ctypes as C
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from welding_robot_amd import api, build, synth


def arg(name, default, n=1, cast=float):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name) + 1
    return cast(sys.argv[i]) if n == 1 else tuple(cast(v) for v in sys.argv[i:i + n])


reps = arg("--reps", 10, cast=int)
WINDOWS = arg("--windows", (1, 16, 128), 3, int)
LIMITS = arg("--limits", (0.25, 1.0, 1.0, 0.5, 0.05, 4.0), 6)
COMPOSED = arg("--composed", 0, cast=int)
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


def once(fn):
    stream = C.c_void_p(ctx.stream)
    ctx.sync()
    hip.hipEventRecord(ev[0], stream)
    out = fn()
    hip.hipEventRecord(ev[1], stream)
    hip.hipEventSynchronize(ev[1])
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
    return out, ms.value


def alternate(title, members, rounds):
    times, outs = {name: [] for name, _ in members}, {}
    for r in range(rounds + 1):
        for name, fn in members:
            if name in outs and outs[name][3] is not None:
                outs[name][3].close()
            outs[name], ms = once(fn)
            if r:
                times[name].append(ms)
    print(title)
    for name, _ in members:
        t = times[name]
        print("    %-44s median %9.3f ms  (min %9.3f, max %9.3f, %d calls)" % (name, np.median(t), min(t), max(t), len(t)))
    return outs


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
curve = api.Trajectory.from_points(ctx, xyz)
v_max, acc, dec, a_lat, v_near, near_d2 = LIMITS
kw = dict(dwell=dwell, a_lat=a_lat, grid=grid, v_near=v_near, near_d2=int(near_d2))
print("C5: %d samples (%d doubled), tick %g s, %d stops of %g s" % (m, N_STOPS, TICK, N_STOPS, DWELL))

members = [("wa_traj_retime_stops", lambda: curve.retime_stops(v_max, acc, dec, TICK, **kw))]
for W in WINDOWS:
    members.append(("wa_traj_retime_jerk, W = %d" % W, lambda W=W: curve.retime_jerk(v_max, acc, dec, TICK, W, **kw)))
o = alternate("whole calls, %d samples:" % m, members, reps)
plain = o["wa_traj_retime_stops"]
print("    unfiltered: %.3f s, %d ticks" % (plain[4]["time_q"] / Q, plain[4]["n_ticks"]))
for W in WINDOWS:
    r = o["wa_traj_retime_jerk, W = %d" % W]
    sj = r[8]
    print("    W = %4d: %s" % (W, sj))
    print("              profile %.3f s; jerk %.4g <= bound %.4g units/s^3; ticks clearance %s" %
          (r[6]["time_q"] / Q, sj["max_d3"] / Q / TICK ** 3, (2.0 * sj["in_max_d2"] / W + 4) / Q / TICK ** 3, r[3].clearance(grid)[3]))
    if W == 1:
        print("              per-sample outputs the bytes of wa_traj_retime_stops: %s" % all(np.array_equal(a, b) for a, b in zip(r[:3], plain[:3])))
for r in o.values():
    if r[3] is not None:
        r[3].close()

if COMPOSED:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jerk_ref as J
    import retime_ref as R

    def composed():
        time_q, w_q, _, ticks, rs, _ = curve.retime_stops(v_max, acc, dec, TICK, ticks=False, **kw)
        L = R._quanta(R.seg_lengths(xyz))
        GL = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        U = J.arcs(xyz, L, GL, time_q, w_q, acc, dec, int(np.rint(TICK * Q)))
        S_q = J.window_means(U, COMPOSED, int(GL[-1]))
        seg, rest, at_end = J.locate(S_q, GL, L, dwell >= 0)
        return None, None, None, api.Trajectory.from_points(ctx, J.positions(xyz, S_q, GL, L, seg, rest, at_end))

    t0 = time.perf_counter()
    out, ms = once(composed)
    print("composed from what exists, W = %d (one call): %.1f ms by the events, %.1f s on the wall; %d ticks" %
          (COMPOSED, ms, time.perf_counter() - t0, len(out[3])))
    out[3].close()
