"""GPU tests of wa_traj_retime_stops, wa_traj_tick_axes_stops and wa_traj_axes_dwells through the C ABI against tests/stops_ref.py (rules
40 - 42 of the header in numpy), bit for bit: every output and every field of every summary.

The scans work on tiles of 2 048 samples; the tick kernel takes 256 ticks per workgroup and 64 per wavefront.  The sizes, the places of
the stops and the lengths of the dwells below stand on both sides of each."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import retime_ref as R
import stops_ref as S
import ticks_ref as K
import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = R.limits(v_max=3, acc=4, dec=6, a_lat=0.7)
TICK = 0.01
DWELL_TICKS = [0.0, 0.3, 5.0, 12.345, 600.0]   # none; no tick may fall inside; whole ticks; a fraction; whole workgroups of ticks inside


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


@pytest.fixture(scope="module")
def slab(ctx):
    grid, xyz, q, tool = K.slab_turn_scene()
    g = grid_of(ctx, grid)
    yield grid, g, xyz, q, tool
    g.close()


@pytest.fixture(scope="module")
def boxes(ctx):
    grid = T.boxes_grid(np.random.RandomState(11), 32, 6)
    g = grid_of(ctx, grid)
    yield grid, g
    g.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stopped_path(n, stops, dwell_ticks=DWELL_TICKS, tick=TICK):
    """n samples of a helix through the 32^3 grid of `boxes` in which the segments `stops` have no length (their sample is doubled) and
    dwell, the lengths of DWELL_TICKS taken in turn; an axis per sample that changes every 7 samples and across every stop.
    Returns (xyz, dwell, q)."""
    stops = sorted(stops)
    src = np.zeros(n, np.int64)
    for i in range(1, n):
        src[i] = src[i - 1] + (0 if i - 1 in stops else 1)
    base = R.helix(max(int(src[-1]) + 1, 2), radius=11.0, pitch=6.0, turns=3.0) + np.array([15.5, 15.5, 3.0], np.float32)
    xyz = base.astype(np.float32)[src]
    dwell = np.full(n - 1, -1.0)
    for k, s in enumerate(stops):
        dwell[s] = dwell_ticks[k % len(dwell_ticks)] * tick
    d = T.quantise_all(T.fib_dirs(32, 2.2, (0.0, 0.0, 1.0)))
    q = d[((src // 7) + 5 * np.cumsum(np.concatenate([[0], dwell >= 0]))) % 32]
    return xyz, dwell, q


def same_retime(ctx, t, xyz, dwell, lim, tick, grid=None, g=None, v_limit=None):
    r = S.retime_stops(xyz, lim, dwell, v_limit, grid, tick)
    args = (lim["v_max"], lim["acc"], lim["dec"], tick)
    kw = dict(dwell=dwell, a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"], v_limit=v_limit)
    time_q, w_q, bound, ticks, s, ss = t.retime_stops(*args, **kw)
    what = (len(xyz), tick, grid is not None, s)
    assert s == r["summary"], (what, r["summary"])
    assert ss == r["stops"], (what, ss, r["stops"])
    assert np.array_equal(w_q, r["w_q"]), (what, np.flatnonzero(w_q != r["w_q"])[:5])
    assert np.array_equal(time_q, r["time_q"]), (what, np.flatnonzero(time_q != r["time_q"])[:5])
    assert np.array_equal(bound, r["bound"]), (what, np.flatnonzero(bound != r["bound"])[:5])
    p = ticks.points()
    assert np.array_equal(bits(p), bits(r["ticks"])), (what, np.flatnonzero((bits(p) != bits(r["ticks"])).any(1))[:5])
    t2, w2, b2, k2, s2, ss2 = t.retime_stops(*args, **kw)      # two calls, the same bytes
    assert s2 == s and ss2 == ss and np.array_equal(t2, time_q) and np.array_equal(w2, w_q) and np.array_equal(b2, bound), what
    assert np.array_equal(bits(k2.points()), bits(p)), what
    for h in (ticks, k2):
        h.close()
    return r, time_q, w_q


def same_tick_axes(ctx, t, xyz, q, time_q, w_q, lim, tick, grid=None, g=None, tool=None, near_add=-1, seg_tag=None, pos=None):
    r = S.tick_axes_stops(xyz, q, time_q, w_q, lim["acc"], lim["dec"], tick, grid, tool, near_add, seg_tag)
    args = (q, time_q, w_q, lim["acc"], lim["dec"], tick)
    kw = dict(seg_tag=seg_tag, grid=g, tool=tool, near_add=near_add)
    axes, blocked, sm, tags, st = t.tick_axes_stops(*args, **kw)
    what = (len(xyz), tick, grid is not None, seg_tag is not None, sm, st)
    assert sm == r["summary"], (what, r["summary"])
    assert st == r["stops"], (what, r["stops"])
    a = axes.points()
    assert np.array_equal(bits(a), bits(r["axes"])), (what, np.flatnonzero((bits(a) != bits(r["axes"])).any(1))[:5])
    assert np.array_equal(blocked, r["blocked"]), (what, np.flatnonzero(blocked != r["blocked"])[:5])
    if seg_tag is None:
        assert tags is None and r["tag"] is None
    else:
        assert np.array_equal(tags, r["tag"]), (what, np.flatnonzero(tags != r["tag"])[:5])
    if pos is not None:   # the positions the restatement checked are the bytes of retime_stops' ticks
        assert np.array_equal(bits(pos), bits(r["pos"])), what
    a2, b2, sm2, tags2, st2 = t.tick_axes_stops(*args, **kw)   # two calls, the same bytes
    assert sm2 == sm and st2 == st and np.array_equal(bits(a2.points()), bits(a)) and np.array_equal(b2, blocked), what
    assert tags is None or np.array_equal(tags2, tags), what
    _, _, sm3, _, st3 = t.tick_axes_stops(*args, axes=False, blocked=False, **kw)
    assert sm3 == sm and st3 == st, what
    for h in (axes, a2):
        h.close()
    return r


def same_dwells(ctx, t, xyz, q, omega, dwell_in=None):
    r = S.axes_dwells(xyz, q, omega, dwell_in)
    out, s = t.axis_dwells(q, omega, dwell_in)
    assert s == r["summary"], (len(xyz), omega, s, r["summary"])
    assert np.array_equal(out.view(np.uint64), r["dwell"].view(np.uint64)), np.flatnonzero(out != r["dwell"])[:5]
    out2, s2 = t.axis_dwells(q, omega, dwell_in)
    assert s2 == s and np.array_equal(out2.view(np.uint64), out.view(np.uint64))
    return r


def stops_for(n):
    if n == 2:
        return [0]                                 # a trajectory that is one dwell and nothing else
    if n == 3:
        return [1]
    if n == 65:
        return [0, 31, 63]
    if n == 4097:
        return [0, 1000, 2046, 2047, 2048, 3000, 4095]   # segment 0, n - 2, three in a row across the tile edge
    return [n // 3, n - 2]


@pytest.mark.parametrize("n", [2, 3, 65, 2048, 2049, 4097])
def test_sample_counts_and_stop_positions(ctx, boxes, n):
    grid, g = boxes
    ticks_of = DWELL_TICKS[4:] + DWELL_TICKS[:4] if n == 2 else (DWELL_TICKS[2:] + DWELL_TICKS[:2] if n in (3, 2048, 2049) else DWELL_TICKS)
    xyz, dwell, q = stopped_path(n, stops_for(n), ticks_of)
    assert len(xyz) == n
    tool = T.rod(9, 16 * 9, 1)
    t = api.Trajectory.from_points(ctx, xyz)
    lim = dict(LIM, v_near=0.8, near_d2=4)
    r, time_q, w_q = same_retime(ctx, t, xyz, dwell, lim, TICK, grid, g)
    assert r["stops"]["n_stops"] == len(stops_for(n))
    tags = (np.arange(n - 1) % 3 * (np.arange(n - 1) % 5 > 0)).astype(np.uint8)   # 0, 1 and 2
    o = same_tick_axes(ctx, t, xyz, q, time_q, w_q, lim, TICK, grid, g, tool, 4, tags, r["ticks"])
    assert o["stops"]["n_dwell_ticks"] > 0
    if n in (2, 4097):                                          # 600 ticks in one dwell: at least one workgroup of 256 lies inside it
        assert o["stops"]["n_dwell_ticks"] >= 600 and (n == 2 or o["stops"]["max_dwell_turn"] > 0)
    same_tick_axes(ctx, t, xyz, q, time_q, w_q, lim, TICK)      # no grid, no tags
    d = same_dwells(ctx, t, xyz, q, 2.0, dwell)
    assert d["summary"]["n_jump"] == len(stops_for(n))
    t.close()


@pytest.mark.parametrize("dwell_ticks", DWELL_TICKS)
def test_dwell_lengths_without_a_grid(ctx, dwell_ticks):
    xyz, dwell, q = stopped_path(200, [70], [dwell_ticks])
    t = api.Trajectory.from_points(ctx, xyz)
    v_limit = np.random.RandomState(3).uniform(0.5, 4.0, len(xyz)).astype(np.float32)
    r, time_q, w_q = same_retime(ctx, t, xyz, dwell, LIM, TICK, v_limit=v_limit)
    tq = r["tick_q"]
    o = same_tick_axes(ctx, t, xyz, q, time_q, w_q, LIM, TICK, seg_tag=(dwell >= 0).astype(np.uint8) * 200, pos=r["ticks"])
    t0, t1 = int(time_q[70]), int(time_q[71])
    assert o["stops"]["n_dwell_ticks"] == -(-t1 // tq) - -(-t0 // tq) == o["stops"]["n_tagged"]
    if dwell_ticks <= 0.3:
        assert o["stops"]["n_dwell_ticks"] <= 1
    t.close()


def test_turn_in_place_over_the_slab(ctx, slab):
    """the 90 degree change of ticks_ref.slab_turn_scene made in place: half way through the dwell the axis points into the metal"""
    grid, g, xyz, q, tool = slab
    cut = int(np.flatnonzero(xyz[:, 0] >= 11.5)[0])
    xyz2 = np.concatenate([xyz[:cut], xyz[cut - 1:]])
    q2 = np.concatenate([q[:cut], q[cut:cut + 1], q[cut:]])
    t = api.Trajectory.from_points(ctx, xyz2)
    d = same_dwells(ctx, t, xyz2, q2, 1.0)
    assert d["summary"]["n_jump"] == d["summary"]["n_stops"] == d["summary"]["n_raised"] == 1 and d["dwell"][cut - 1] > 1.4
    lim = R.limits(v_max=3, acc=4, dec=6, a_lat=0.7, v_near=0.5, near_d2=9)
    r, time_q, w_q = same_retime(ctx, t, xyz2, d["dwell"], lim, TICK, grid, g)
    assert r["summary"]["n_bound"][3] > 0
    o = same_tick_axes(ctx, t, xyz2, q2, time_q, w_q, lim, TICK, grid, g, tool, 3, pos=r["ticks"])
    assert o["stops"]["n_dwell_ticks"] > 140 and 0 < o["summary"]["n_blocked"] < o["stops"]["n_dwell_ticks"]
    assert o["blocked"][o["dwell"]].sum() == o["summary"]["n_blocked"]          # blocked only while it turns
    t.close()


def test_reductions_on_the_device(ctx, boxes):
    grid, g = boxes
    xyz, _, q = stopped_path(2500, [100, 2047])                  # two doubled samples, no duration
    tool = T.rod(9, 16 * 9, 1)
    t = api.Trajectory.from_points(ctx, xyz)
    lim = dict(LIM, v_near=0.8, near_d2=4)
    args = (lim["v_max"], lim["acc"], lim["dec"], TICK)
    kw = dict(a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"])
    a = t.retime(*args, **kw)
    b = t.retime_stops(*args, dwell=None, **kw)
    c = t.retime_stops(*args, dwell=np.full(len(xyz) - 1, -1.0), **kw)
    for o in (b, c):
        assert o[4] == a[4] and o[5] == dict(n_stops=0, n_stop_samples=0, dwell_q=0)
        assert all(np.array_equal(o[k], a[k]) for k in range(3)) and np.array_equal(bits(o[3].points()), bits(a[3].points()))
    time_q, w_q = a[0], a[1]
    axes, blocked, sm = t.tick_axes(q, time_q, w_q, lim["acc"], lim["dec"], TICK, g, tool, 4)
    axes2, blocked2, sm2, tags, st = t.tick_axes_stops(q, time_q, w_q, lim["acc"], lim["dec"], TICK, grid=g, tool=tool, near_add=4)
    assert sm2 == sm and st == dict(n_dwell_ticks=0, n_tagged=0, max_dwell_turn=0) and tags is None
    assert np.array_equal(bits(axes2.points()), bits(axes.points())) and np.array_equal(blocked2, blocked)
    for h in (a[3], b[3], c[3], axes, axes2, t):
        h.close()


def test_what_is_refused_leaves_the_outputs_alone(ctx):
    xyz, dwell, q = stopped_path(100, [40], [5.0])
    n = len(xyz)
    t = api.Trajectory.from_points(ctx, xyz)
    lim = L.RetimeLimits(3.0, 4.0, 6.0, float("inf"), 0.0, -1)
    q32 = np.ascontiguousarray(q, np.int32)

    def retime_refused(d):
        time_q, w_q, bound = np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(n, 77, np.uint8)
        th, s, s2 = C.c_void_p(), L.RetimeSummary(), L.StopsSummary()
        s.n, s2.n_stops = -7, -7
        d = np.ascontiguousarray(d, np.float64)
        rc = ctx.lib.wa_traj_retime_stops(None, t.h, C.byref(lim), None, d.ctypes.data, C.c_double(TICK), time_q.ctypes.data, w_q.ctypes.data,
                                          bound.ctypes.data, C.byref(th), C.byref(s), C.byref(s2))
        assert rc == 1 and not th.value and s.n == -7 and s2.n_stops == -7, (rc, d[38:42])
        assert (time_q == -7).all() and (w_q == -7).all() and (bound == 77).all()

    def dwells_refused(d, omega=1.0):
        out = np.full(n - 1, -7.0)
        s = L.AxesDwellsSummary()
        s.n = -7
        d = np.ascontiguousarray(d, np.float64)
        rc = ctx.lib.wa_traj_axes_dwells(t.h, q32.ctypes.data, C.c_double(omega), d.ctypes.data, out.ctypes.data, C.byref(s))
        assert rc == 1 and s.n == -7 and (out == -7.0).all(), (rc, omega)

    for bad in (np.nan, np.inf, -np.inf, float(1 << 31)):
        d = dwell.copy()
        d[40] = bad
        retime_refused(d)
        with pytest.raises(ValueError):
            S.retime_stops(xyz, R.limits(v_max=3, acc=4, dec=6), d)
    d = dwell.copy()
    d[3] = 0.0                                                   # a stop on a segment that has a length
    retime_refused(d)
    dwells_refused(d)
    for bad in (np.nan, np.inf):
        d = dwell.copy()
        d[40] = bad
        dwells_refused(d)
    for omega in (0.0, -1.0, np.inf, np.nan):
        dwells_refused(dwell, omega)
    # tags out without tags in, and a missing stops summary
    time_q, w_q, _, _, _, _ = t.retime_stops(3.0, 4.0, 6.0, TICK, dwell=dwell, ticks=False)
    tag_out = np.full(10, 77, np.uint8)
    s, s2 = L.TickAxesSummary(), L.TickStopsSummary()
    s.n_ticks = -7
    rc = ctx.lib.wa_traj_tick_axes_stops(None, t.h, q32.ctypes.data, None, -1, C.c_double(4.0), C.c_double(6.0), C.c_double(TICK), time_q.ctypes.data,
                                         w_q.ctypes.data, None, None, None, tag_out.ctypes.data, C.byref(s), C.byref(s2))
    assert rc == 1 and s.n_ticks == -7 and (tag_out == 77).all()
    rc = ctx.lib.wa_traj_tick_axes_stops(None, t.h, q32.ctypes.data, None, -1, C.c_double(4.0), C.c_double(6.0), C.c_double(TICK), time_q.ctypes.data,
                                         w_q.ctypes.data, None, None, None, None, C.byref(s), None)
    assert rc == 1 and s.n_ticks == -7
    t.close()


def test_plan_batch_weld_passes():
    """examples/plan_batch.py --seams --weld-passes ends with the weld_passes report; the run without the flag prints what it printed"""
    base = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "32", "--points", "6", "--exact-paths", "--shortcut", "--seams"]
    a = subprocess.run(base + ["--weld-passes", "0.5", "0.2", "0.1"], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stdout[-800:] + a.stderr[-2000:]
    ra = json.loads(a.stdout.strip().splitlines()[-1])
    wp = ra["weld_passes"]
    assert wp["n_stops"] == 6
    assert abs(wp["dwell_s"] - 3 * 0.3) <= 6 / api.RETIME_Q      # one quantum per stop
    assert wp["seam_length"] > 0 and wp["weld_s"] >= wp["seam_length"] / 0.5
    assert wp["weld_ticks"] > 0 and wp["n_ticks"] > wp["weld_ticks"]
    assert abs(wp["duration_s"] - (wp["dwell_s"] + wp["weld_s"] + wp["travel_s"])) < 1e-9
    b = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-800:] + b.stderr[-2000:]
    rb = json.loads(b.stdout.strip().splitlines()[-1])
    assert "weld_passes" not in rb

    def results(d):   # everything but the wall-clock figures and the new report
        if isinstance(d, dict):
            return {k: results(v) for k, v in d.items() if not (k.startswith("t_") or k.endswith("_per_s") or k == "weld_passes")}
        return d
    assert results(ra) == results(rb)
