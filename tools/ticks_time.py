#!/usr/bin/env python3
"""Time the tool poses at controller ticks (wa_traj_axes_smooth, wa_traj_axes_limits, wa_traj_tick_axes) on C5's tour: 256^3
synth_grid, 64 points, --exact-paths --shortcut --fit at 100 001 samples, the torch stage of examples/plan_batch.py with K directions,
then axes -> smooth -> limits -> retime with that limit -> tick axes.  Whole calls by HIP events on the context's stream, one warm-up,
median and range.  The yardstick is the composition the calls replace: time_q / w_q are on the host anyway (wa_traj_retime returned
them), the tick axes are computed from them in numpy by the definition's vectorised form (below) and uploaded with
wa_traj_from_points; the check of the uploaded axes against the metal (wa_traj_tool_check on retime's tick positions) is timed apart.
Both must end on the same bytes.  Kernel times: run it alone under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/ticks_time.py --reps 3 --no-composed`.

    python tools/ticks_time.py [--reps N] [--K 64] [--omega 2.0] [--limits V_MAX ACC DEC A_LAT V_NEAR NEAR_D2] [--no-composed]
                               [--retime-lib PATH]     (another build of the library, e.g. the parent commit's: wa_traj_retime for scale)"""
import ctypes as C
import importlib.util
import os
import sys

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
K = arg("--K", 64, cast=int)
omega = arg("--omega", 2.0)
LIMITS = arg("--limits", (0.25, 1.0, 1.0, 0.5, 0.05, 4.0), 6)
TICK = 0.001
spec = importlib.util.spec_from_file_location("plan_batch", os.path.join(ROOT, "examples", "plan_batch.py"))
pb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pb)
hip = C.CDLL(os.path.join(build.rocm_lib_dir(), "libamdhip64.so"))
ctx = api.Context(0)
print("device:", ctx.device_name)
ev = [C.c_void_p(), C.c_void_p()]
assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0
Q, QF = 1 << 30, np.float64(1 << 30)


def timed(fn, c=ctx, n=None):
    out, times = None, []
    stream = C.c_void_p(c.stream)
    for r in range((reps if n is None else n) + 1):          # the first call warms up
        c.sync()
        hip.hipEventRecord(ev[0], stream)
        out = fn()
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        if r:
            times.append(ms.value)
    return out, float(np.median(times)), "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(times), min(times), max(times), len(times))


def host_tick_axes(p32, q, time_q, B, acc, dec, tick):
    """rule 26's axes on the host: rule 6's segment and lambda per tick, the interpolated axis, rule 1"""
    p = p32.astype(np.float64)
    n = len(p)
    d = p[1:] - p[:-1]
    ds = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    L = np.rint(ds * QF).astype(np.int64)
    v = np.sqrt(B.astype(np.float64) / QF)
    vs = v[:-1] + v[1:]
    tri = (L > 0) & (vs == 0)
    wp = (((2.0 * ds) * acc) * dec) / (acc + dec)
    t_up = np.sqrt(wp) / acc
    with np.errstate(all="ignore"):
        dt = np.where(tri, t_up + np.sqrt(wp) / dec, np.where(L > 0, (2.0 * ds) / vs, 0.0))
    total, tick_q = int(time_q[-1]), int(np.rint(tick * QF))
    taus = np.arange(total // tick_q + 1, dtype=np.int64) * tick_q
    if total % tick_q:
        taus = np.concatenate([taus, [total]])
    i = np.searchsorted(time_q[:n - 1], taus, side="right") - 1
    e = (taus - time_q[i]).astype(np.float64) / QF
    with np.errstate(all="ignore"):
        a = ((B[i + 1] - B[i]).astype(np.float64) / QF) / (2.0 * ds[i])
        r = dt[i] - e
        s = np.where(tri[i], np.where(e <= t_up[i], ((0.5 * acc) * e) * e, ds[i] - ((0.5 * dec) * r) * r), (v[i] * e) + ((0.5 * a) * e) * e)
        lam = np.clip(np.nan_to_num(s / ds[i]), 0.0, 1.0)
    lam = np.where(taus >= time_q[i + 1], 1.0, np.where(L[i] == 0, 0.0, lam))
    qa, qb = q[i].astype(np.float64), q[i + 1].astype(np.float64)
    w = qa + (qb - qa) * lam[:, None]
    ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    zero = ln == 0
    with np.errstate(all="ignore"):
        qt = np.rint((w / ln[:, None]) * 16384.0)
    qt[zero] = qa[zero]
    return (qt.astype(np.int64) / 16384.0).astype(np.float32)   # (through the integers: rint gives -0.0 for a small negative, the axis has +0.0)


# ---- C5's tour and its torch stage
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
xyz = samples.points()
segs = [paths[(min(a, b), max(a, b))] for a, b in edges]
first = np.asarray([(s[-1] if r else s[0]) for s, r in zip(segs, rev)] + [segs[-1][0] if rev[-1] else segs[-1][-1]], np.int64)
stops = np.stack([cx[first % grid.nx], cy[(first // grid.nx) % grid.ny], cz[first // (grid.nx * grid.ny)]], 1)
info = pb.torch_stage(ctx, grid, xyz, stops, K)
off, chosen, dirs, tool = pb.torch_stage.last
q0 = api.quantise_axes(dirs)[chosen]
print("C5: %d samples, %d legs, K = %d, %d directions used, %d samples with a blocked direction" %
      (len(xyz), len(off) - 1, K, info["directions_used"], info["n_chosen_blocked"]))
v_max, acc, dec, a_lat, v_near, near_d2 = LIMITS
h = 8.0 * float(grid.precision)
kw = dict(a_lat=a_lat, grid=grid, v_near=v_near, near_d2=int(near_d2))

sm, _, t_smooth = timed(lambda: samples.smooth_axes(q0, h, 8, grid, tool, off))
print("wa_traj_axes_smooth (h = %g, max_level 8): %s\n    %s" % (h, t_smooth, sm["summary"]))
(v_limit, ls), _, t_lim = timed(lambda: samples.axis_limits(sm["q"], omega, v_max, v_max * 1e-3))
print("wa_traj_axes_limits (omega = %g): %s\n    %s" % (omega, t_lim, ls))
free_run, _, t_free = timed(lambda: samples.retime(v_max, acc, dec, TICK, ticks=True, **kw))
print("wa_traj_retime without the turn limit, this build: %s; duration %.3f s, %d ticks" % (t_free, free_run[4]["time_q"] / Q, free_run[4]["n_ticks"]))
if "--retime-lib" in sys.argv:
    from welding_robot_amd import _lib
    held = dict(_lib.SYMBOLS)                                  # an older build lacks the newest entry points: declare what it has
    probe = C.CDLL(sys.argv[sys.argv.index("--retime-lib") + 1])
    for name in list(_lib.SYMBOLS):
        if not hasattr(probe, name):
            del _lib.SYMBOLS[name]
    other = api.Context(0, lib_path=sys.argv[sys.argv.index("--retime-lib") + 1])
    _lib.SYMBOLS.update(held)
    og = api.Grid.from_occupancy(other, free, cx, cy, cz, prec, wall)
    ot = api.Trajectory.from_points(other, xyz)
    okw = dict(kw, grid=og)
    o_run, _, t_other = timed(lambda: ot.retime(v_max, acc, dec, TICK, ticks=True, **okw), other)
    same = all(np.array_equal(a, b) for a, b in zip(o_run[:3], free_run[:3])) and o_run[3].points().tobytes() == free_run[3].points().tobytes()
    print("wa_traj_retime without the turn limit, %s: %s; same bytes: %s" % (sys.argv[sys.argv.index("--retime-lib") + 1], t_other, same))
run, _, t_rt = timed(lambda: samples.retime(v_max, acc, dec, TICK, v_limit=v_limit, ticks=False, **kw))
print("wa_traj_retime with the turn limit, without its ticks: %s; duration %.3f s, %d ticks" % (t_rt, run[4]["time_q"] / Q, run[4]["n_ticks"]))
# the tick axes are timed on the timing WITHOUT the turn limit: the tick count of the README's row for wa_traj_retime
time_q, w_q, _, tick_pos, rs = free_run
(axes, blocked, ts), ms, t_ticks = timed(lambda: samples.tick_axes(sm["q"], time_q, w_q, acc, dec, TICK, grid, tool, near_add=8))
print("wa_traj_tick_axes (axes on the device, one byte per tick to the host): %s\n    %s" % (t_ticks, ts))
(_, _, ts2), ms2, t_ticks2 = timed(lambda: samples.tick_axes(sm["q"], time_q, w_q, acc, dec, TICK, grid, tool, near_add=8, blocked=False))
print("wa_traj_tick_axes (axes on the device, summary only): %s" % t_ticks2)
out_bytes = ts["n_ticks"] * 13
print("    bytes out per tick 12 (axis) + 1 (blocked): %.1f MB; over the whole call without the byte copy %.1f GB/s = %.2f %% of 8 TB/s "
      "(the call also uploads q, time_q, w_q and waits for its summary; the kernel's own time: rocprofv3)" %
      (out_bytes / 1e6, out_bytes / ms2 / 1e6, 100 * out_bytes / ms2 / 1e6 / 8000))
if "--no-composed" not in sys.argv:
    def composed():
        a = host_tick_axes(xyz, sm["q"].astype(np.int64), time_q, w_q, acc, dec, TICK)
        return a, api.Trajectory.from_points(ctx, a)
    (host_axes, up), _, t_comp = timed(composed, n=min(reps, 3))
    print("composed (numpy from the read-back time_q / w_q, upload of the axes): %s; same bytes: %s" %
          (t_comp, host_axes.tobytes() == axes.points().tobytes()))
    (cb, _, cs), _, t_check = timed(lambda: tick_pos.torch_check(grid, host_axes, tool, 8), n=min(reps, 3))
    print("    + wa_traj_tool_check of those axes at retime's tick positions (axes through the host again): %s; blocked bytes that differ: %d "
          "(the check quantises the floats a second time, which can move a component by 1)" % (t_check, int((cb != blocked).sum())))
