"""GPU tests of wa_traj_axes_smooth, wa_traj_axes_limits and wa_traj_tick_axes through the C ABI against tests/ticks_ref.py (rules 24 - 26
of the header in numpy), bit for bit: every output and every field of the three summaries.

The scans of rule 24 work on tiles of 2 048 samples and gain a level at 2 049 and at 2^22 + 1; the tick kernel takes 256 ticks per
workgroup and 64 per wavefront.  The sizes below stand on both sides of each."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import retime_ref as R
import ticks_ref as K
import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = R.limits(v_max=3, acc=4, dec=6, a_lat=0.7)


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


def path_in_boxes(n, seed=0):
    """n samples of a helix through the 32^3 grid of `boxes`, a few of them outside the coordinate range"""
    xyz = R.helix(n, radius=11.0, pitch=6.0, turns=3.0) + np.array([15.5, 15.5, 3.0], np.float32)
    if seed:
        xyz[:3, 0] -= 30.0
    return xyz.astype(np.float32)


def same_smooth(ctx, xyz, q, h, max_level, grid=None, g=None, tool=None, off=None):
    r = K.smooth(xyz, q, h, max_level, grid, tool, off)
    t = api.Trajectory.from_points(ctx, xyz)
    o = t.smooth_axes(q, h, max_level, g, tool, off)
    what = (len(xyz), h, max_level, grid is not None, None if off is None else list(off)[:6])
    assert o["summary"] == r["summary"], (what, o["summary"], r["summary"])
    assert np.array_equal(o["q"], r["q"]), (what, np.flatnonzero((o["q"] != r["q"]).any(1))[:5])
    assert np.array_equal(o["level"], r["level"]) and np.array_equal(o["blocked"], r["blocked"]), what
    o2 = t.smooth_axes(q, h, max_level, g, tool, off)         # two calls, the same bytes
    assert o2["summary"] == o["summary"] and all(np.array_equal(o2[k], o[k]) for k in ("q", "level", "blocked")), what
    t.close()
    return r


def same_limits(ctx, xyz, q, omega, v_cap, v_floor, v_in=None):
    r = K.limits(xyz, q, omega, v_cap, v_floor, v_in)
    t = api.Trajectory.from_points(ctx, xyz)
    f, s = t.axis_limits(q, omega, v_cap, v_floor, v_in)
    assert s == r["summary"], (len(xyz), omega, s, r["summary"])
    assert np.array_equal(bits(f), bits(r["v_limit"])), np.flatnonzero(bits(f) != bits(r["v_limit"]))[:5]
    f2, s2 = t.axis_limits(q, omega, v_cap, v_floor, v_in)
    assert s2 == s and np.array_equal(bits(f2), bits(f))
    t.close()
    return r


def same_ticks(ctx, xyz, q, lim=LIM, tick=0.01, grid=None, g=None, tool=None, near_add=-1, v_limit=None):
    """retime on the device, then the tick axes of its result against the restatement run on the SAME time_q / w_q"""
    t = api.Trajectory.from_points(ctx, xyz)
    time_q, w_q, _, ticks, s = t.retime(lim["v_max"], lim["acc"], lim["dec"], tick, a_lat=lim["a_lat"], v_limit=v_limit)
    r = K.tick_axes(xyz, q, time_q, w_q, lim["acc"], lim["dec"], tick, grid, tool, near_add)
    axes, blocked, sm = t.tick_axes(q, time_q, w_q, lim["acc"], lim["dec"], tick, g, tool, near_add)
    what = (len(xyz), tick, grid is not None, s["n_ticks"])
    assert sm == r["summary"], (what, sm, r["summary"])
    assert sm["n_ticks"] == s["n_ticks"] == len(axes)
    a = axes.points()
    assert np.array_equal(bits(a), bits(r["axes"])), (what, np.flatnonzero((bits(a) != bits(r["axes"])).any(1))[:5])
    assert np.array_equal(blocked, r["blocked"]), (what, np.flatnonzero(blocked != r["blocked"])[:5])
    # retime agreement: the positions the restatement checked are the bytes of retime's ticks_out
    assert np.array_equal(bits(ticks.points()), bits(r["pos"])), what
    a2, b2, sm2 = t.tick_axes(q, time_q, w_q, lim["acc"], lim["dec"], tick, g, tool, near_add)
    assert sm2 == sm and np.array_equal(bits(a2.points()), bits(a)) and np.array_equal(b2, blocked), what
    _, _, sm3 = t.tick_axes(q, time_q, w_q, lim["acc"], lim["dec"], tick, g, tool, near_add, axes=False, blocked=False)
    assert sm3 == sm, what
    for h in (axes, a2, ticks, t):
        h.close()
    return r, time_q, w_q


@pytest.mark.parametrize("n", [2, 3, 2047, 2048, 2049, 4097])
def test_sample_counts_around_the_scan_tile(ctx, boxes, n):
    grid, g = boxes
    xyz = path_in_boxes(n, seed=1 if n > 3 else 0)
    q = K.stepped_axes(n, every=7, K=32, half_angle=2.2)
    tool = T.rod(9, 16 * 9, 1)
    r = same_smooth(ctx, xyz, q, 3.0, 8, grid, g, tool)
    if n > 3:
        assert r["summary"]["n_outside"] == 3
    same_smooth(ctx, xyz, q, 3.0, 8)                           # g == NULL
    same_limits(ctx, xyz, q, 3.0, 3.0, 1e-3)
    same_limits(ctx, xyz, r["q"], 0.5, 3.0, 1e-3, np.random.RandomState(n).uniform(0.2, 4.0, n).astype(np.float32))
    same_ticks(ctx, xyz, r["q"], tick=0.05, grid=grid, g=g, tool=tool, near_add=4)


def test_two_to_the_22_plus_one_samples_without_a_grid(ctx):
    n = (1 << 22) + 1                                          # the scans' third level; two legs, a leg holds at most 2^22 samples
    xyz = R.helix(n, radius=0.5, pitch=0.05, turns=40.0)
    q = K.stepped_axes(n, every=4099, K=32)
    r = K.smooth(xyz, q, 0.01, 2, off=[0, 1 << 22, n])
    t = api.Trajectory.from_points(ctx, xyz)
    o = t.smooth_axes(q, 0.01, 2, off=[0, 1 << 22, n])
    assert o["summary"] == r["summary"] and np.array_equal(o["q"], r["q"]) and not o["level"].any() and not o["blocked"].any()
    with pytest.raises(api.WeldacsError) as e:
        t.smooth_axes(q, 0.01, 2)                              # one leg of 2^22 + 1
    assert e.value.code == 7
    t.close()


def test_leg_boundaries(ctx, slab):
    grid, g, xyz, q, tool = slab
    n = len(xyz)
    cut = int(np.flatnonzero(xyz[:, 0] >= 11.5)[0])
    r = same_smooth(ctx, xyz, q, 2.0, 8, grid, g, tool, off=[0, cut, n])   # the boundary on the change: no window sees both axes
    assert np.array_equal(r["q"], K.quantise_rows(q.astype(np.float64))) and r["summary"]["max_turn_out"] == 0
    same_smooth(ctx, xyz, q, 2.0, 8, grid, g, tool, off=[0, cut - 2, n])  # a boundary inside the windows around the change
    same_smooth(ctx, xyz, q, 2.0, 8, grid, g, tool, off=[0, 0, cut - 2, cut - 2, cut - 2, n, n])   # empty legs, first and last included
    same_smooth(ctx, xyz, q, 2.0, 3, off=[0, 1, 2, n])                    # legs of one sample, no grid


def test_zero_length_segments_and_cancelling_axes(ctx, boxes):
    grid, g = boxes
    xyz = np.repeat(path_in_boxes(40), 3, 0)                   # every sample three times: GL stands still twice in a row
    xyz[-4:] = xyz[-4]
    q = K.stepped_axes(len(xyz), every=5, K=16, half_angle=2.8)
    tool = T.rod(5, 16 * 8, 2)
    same_smooth(ctx, xyz, q, 0.0, 8, grid, g, tool)            # h = 0: a window is the samples that share the place
    r = same_smooth(ctx, xyz, q, 4.0, 4, grid, g, tool)
    lim = same_limits(ctx, xyz, q, 1.0, 2.0, 0.05)
    assert lim["summary"]["n_jump"] > 0
    same_ticks(ctx, xyz, r["q"], lim=R.limits(v_max=6, acc=9, dec=9), tick=0.1, grid=grid, g=g, tool=tool, v_limit=lim["v_limit"])
    two = np.array([[3, 3, 3], [3.5, 3, 3]], np.float32)       # antipodal neighbours: S = 0 in the window, v = 0 at lambda = 1/2
    qa = np.array([[0, 0, 16384], [0, 0, -16384]])
    r = same_smooth(ctx, two, qa, 1.0, 4)
    assert r["summary"]["n_zero_sum"] == 2 and np.array_equal(r["q"], qa)
    same_smooth(ctx, two, qa, 1.0, 4, grid, g, tool)


@pytest.mark.parametrize("max_level", [0, 3, 8])
def test_level_climbing_on_the_slab(ctx, slab, max_level):
    grid, g, xyz, q, tool = slab
    r = same_smooth(ctx, xyz, q, 2.0, max_level, grid, g, tool)
    if max_level:
        assert any(r["summary"]["n_level"][1:]), r["summary"]  # the level really climbs
    long_rod = T.rod(64, 16 * 20, 9)                           # 64 beads that reach the slab from everywhere above it: blocked at every level
    r = same_smooth(ctx, xyz, q, 2.0, max_level, grid, g, long_rod)
    assert r["summary"]["n_blocked"] > 0 and r["summary"]["n_level"][max_level] >= r["summary"]["n_blocked"]
    assert r["summary"]["first_blocked"] == int(np.flatnonzero(r["blocked"])[0])


def test_a_grid_without_obstacles(ctx):
    grid = T.make_grid(np.ones((8, 8, 8), np.uint8), (8, 8, 8))
    g = grid_of(ctx, grid)
    xyz = (R.helix(300, radius=3.0, pitch=1.0) + np.array([3.5, 3.5, 2.0])).astype(np.float32)
    q = K.stepped_axes(300)
    r = same_smooth(ctx, xyz, q, 0.5, 8, grid, g, T.rod(4))
    assert r["summary"]["n_level"][0] == 300
    r, _, _ = same_ticks(ctx, xyz, r["q"], grid=grid, g=g, tool=T.rod(4), near_add=50)
    assert r["summary"]["n_blocked"] == 0 and r["summary"]["n_near"] == 0
    g.close()


def _tick_for(ctx, xyz, lim, want):
    """a tick period that gives exactly `want` ticks on xyz under lim (the duration from a first retime)"""
    t = api.Trajectory.from_points(ctx, xyz)
    time_q = t.retime(lim["v_max"], lim["acc"], lim["dec"], 1.0, a_lat=lim["a_lat"], ticks=False)[0]
    t.close()
    total = int(time_q[-1])
    tick_q = total // (want - 1)                               # want - 1 full periods and a rest below one period, or none
    while R.tick_count(total, tick_q) > want:
        tick_q += 1
    assert R.tick_count(total, tick_q) == want
    return tick_q / R.Q


@pytest.mark.parametrize("want", [2, 255, 256, 257, 300001])
def test_tick_counts(ctx, boxes, want):
    grid, g = boxes
    n = 700
    xyz = path_in_boxes(n, seed=1)
    q = K.stepped_axes(n, every=9, K=32, half_angle=2.2)
    tool = T.rod(6, 16 * 7, 1)
    r, _, _ = same_ticks(ctx, xyz, q, tick=_tick_for(ctx, xyz, LIM, want), grid=grid, g=g, tool=tool, near_add=6)
    assert r["summary"]["n_ticks"] == want and r["summary"]["max_tick_turn"] > 0
    if want > 255:
        assert r["summary"]["n_blocked"] > 0 and r["summary"]["n_near"] > 0 and r["summary"]["n_outside"] > 0


def test_one_tick_and_a_tick_longer_than_the_duration(ctx, boxes):
    grid, g = boxes
    tool = T.rod(3)
    q5 = K.stepped_axes(5, every=1)
    r, _, _ = same_ticks(ctx, np.full((5, 3), 4.0, np.float32), q5, grid=grid, g=g, tool=tool)   # no length at all: one tick
    assert r["summary"]["n_ticks"] == 1 and r["summary"]["max_tick_turn"] == 0 and np.array_equal(r["qt"][0], q5[-1])
    r, _, _ = same_ticks(ctx, path_in_boxes(11), K.stepped_axes(11, every=2), tick=1000.0, grid=grid, g=g, tool=tool)
    assert r["summary"]["n_ticks"] == 2


def test_tick_details(ctx, boxes):
    grid, g = boxes
    # a tick exactly on a sample time: times chosen by hand (they need not come from retime, rule 26 takes them as given)
    xyz = np.array([[4, 4, 4], [5, 4, 4], [6, 4, 4], [6, 4, 4], [7, 4, 4]], np.float32)
    q = np.array([[0, 0, 16384], [0, 16384, 0], [16384, 0, 0], [0, -16384, 0], [0, 0, -16384]])
    time_q = np.array([0, 4, 8, 8, 12], np.int64) * (R.Q // 4)
    w_q = np.array([0, 1, 1, 1, 0], np.int64) * R.Q
    t = api.Trajectory.from_points(ctx, xyz)
    for tick in (0.25, 1.0, 0.375, 2.0 ** -12):
        r = K.tick_axes(xyz, q, time_q, w_q, 2.0, 2.0, tick, grid, T.rod(3), 2)
        axes, blocked, s = t.tick_axes(q, time_q, w_q, 2.0, 2.0, tick, g, T.rod(3), 2)
        assert s == r["summary"] and np.array_equal(bits(axes.points()), bits(r["axes"])) and np.array_equal(blocked, r["blocked"]), tick
        axes.close()
    r = K.tick_axes(xyz, q, time_q, w_q, 2.0, 2.0, 1.0)
    assert r["qt"].tolist()[:4] == [[0, 0, 16384], [0, 16384, 0], [0, -16384, 0], [0, 0, -16384]]   # on a sample time: the sample's own axis
    t.close()
    # antipodal neighbours: v = 0 at lambda = 1/2 exactly (a segment at constant speed, the tick half-way in time)
    two = np.array([[4, 4, 4], [5, 4, 4]], np.float32)
    qa = np.array([[0, 0, 16384], [0, 0, -16384]])
    t = api.Trajectory.from_points(ctx, two)
    tq, wq = np.array([0, R.Q], np.int64), np.array([R.Q, R.Q], np.int64)
    r = K.tick_axes(two, qa, tq, wq, 1.0, 1.0, 0.5)
    assert r["lam"].tolist() == [0.0, 0.5, 1.0] and r["qt"].tolist() == [[0, 0, 16384], [0, 0, 16384], [0, 0, -16384]]
    axes, blocked, s = t.tick_axes(qa, tq, wq, 1.0, 1.0, 0.5)
    assert s == r["summary"] and np.array_equal(bits(axes.points()), bits(r["axes"])) and not blocked.any()
    axes.close()
    t.close()
    # K = 1 (one direction for every sample) and a 64-bead tool
    xyz = path_in_boxes(500)
    q1 = K.stepped_axes(500, every=7, K=1)
    r, _, _ = same_ticks(ctx, xyz, q1, grid=grid, g=g, tool=T.rod(64, 16 * 12, 3), near_add=9)
    assert r["summary"]["max_tick_turn"] == 0 and (r["qt"] == q1[0]).all()
    same_smooth(ctx, xyz, q1, 1.0, 8, grid, g, T.rod(64, 16 * 12, 3))


def _raw(ctx, name, *args):
    return getattr(ctx.lib, name)(*args)


def test_errors_leave_the_outputs_untouched(ctx, boxes):
    grid, g = boxes
    n = 40
    xyz = path_in_boxes(n)
    q = K.stepped_axes(n).astype(np.int32)
    t = api.Trajectory.from_points(ctx, xyz)
    tool = api.torch_tool(*T.rod(4))
    off = np.array([0, n], np.int64)
    P = lambda a: a.ctypes.data if a is not None else None
    bad_xyz = xyz.copy()
    bad_xyz[7, 1] = np.inf
    t_bad = api.Trajectory.from_points(ctx, bad_xyz)
    huge = np.zeros((3, 3), np.float32)
    huge[1, 0] = 3e9
    huge[2, 0] = -3e9                                          # two segments of 3e9 and 6e9: L sums to more than 2^61 / 2^30 = 2^31
    t_huge = api.Trajectory.from_points(ctx, huge)

    def smooth(tr=t, qq=q, tl=tool, gg=g, of=off, h=1.0, ml=3, nl=None):
        qo, lv, bl = np.full((len(qq), 3), 77, np.int32), np.full(len(qq), 77, np.uint8), np.full(len(qq), 77, np.uint8)
        s = L.AxesSmoothSummary()
        s.n = -5
        rc = _raw(ctx, "wa_traj_axes_smooth", gg.h if gg else None, tr.h, P(qq), C.byref(tl) if tl else None, P(of),
                  len(of) - 1 if nl is None else nl, C.c_double(h), ml, P(qo), P(lv), P(bl), C.byref(s))
        assert (qo == 77).all() and (lv == 77).all() and (bl == 77).all() and s.n == -5
        return rc

    q_big, q_zero = q.copy(), q.copy()
    q_big[3, 2] = 16385
    q_zero[5] = 0
    beads_bad = api.torch_tool([0, 70000], [1, 1])
    for kw in (dict(h=-1.0), dict(h=np.nan), dict(h=np.inf), dict(h=2.0 ** 31 + 1024), dict(ml=-1), dict(ml=9), dict(qq=q_big), dict(qq=q_zero),
               dict(tl=None), dict(gg=None), dict(of=np.array([0, 10, 5, n], np.int64)), dict(of=np.array([1, n], np.int64)),
               dict(of=np.array([0, n - 1], np.int64)), dict(nl=0), dict(tl=beads_bad), dict(tr=t_bad),
               dict(tr=t_huge, qq=q[:3], of=np.array([0, 3], np.int64), gg=None, tl=None)):
        assert smooth(**kw) == 1, kw

    def limits(tr=t, qq=q, omega=1.0, cap=2.0, floor=0.1, vin=None):
        out = np.full(len(qq), 77.0, np.float32)
        s = L.AxesLimitsSummary()
        s.n = -5
        rc = _raw(ctx, "wa_traj_axes_limits", tr.h, P(qq), C.c_double(omega), C.c_double(cap), C.c_double(floor), P(vin), P(out), C.byref(s))
        assert (out == 77.0).all() and s.n == -5
        return rc

    vin_bad = np.ones(n, np.float32)
    vin_bad[n - 1] = 0.0
    vin_nan = np.ones(n, np.float32)
    vin_nan[0] = np.nan
    for kw in (dict(omega=0.0), dict(omega=np.inf), dict(omega=np.nan), dict(cap=0.0), dict(cap=-1.0), dict(cap=np.inf), dict(floor=0.0),
               dict(floor=np.nan), dict(floor=3.0), dict(cap=1e300, floor=1e200), dict(vin=vin_bad), dict(vin=vin_nan), dict(qq=q_big),
               dict(qq=q_zero), dict(tr=t_bad)):
        assert limits(**kw) == 1, kw

    time_q, w_q, _, _, _ = t.retime(1.0, 2.0, 2.0, 0.01, ticks=False)

    def ticks(tr=t, qq=q, tl=tool, gg=g, near=3, acc=2.0, dec=2.0, tick=0.01, tq=time_q, wq=w_q, expect_handle=77):
        bl = np.full(1 << 16, 77, np.uint8)
        th = C.c_void_p(77)
        s = L.TickAxesSummary()
        s.n_ticks = -5
        rc = _raw(ctx, "wa_traj_tick_axes", gg.h if gg else None, tr.h, P(qq), C.byref(tl) if tl else None, near, C.c_double(acc), C.c_double(dec),
                  C.c_double(tick), P(tq), P(wq), C.byref(th), P(bl), C.byref(s))
        assert (bl == 77).all() and s.n_ticks == -5 and th.value == expect_handle
        return rc

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    for kw in (dict(acc=0.0), dict(dec=np.inf), dict(acc=np.nan), dict(tick=np.nan), dict(tick=0.0), dict(tick=2.0 ** 32), dict(tl=None),
               dict(gg=None), dict(near=(1 << 30) + 1), dict(tl=beads_bad), dict(qq=q_big), dict(qq=q_zero), dict(tr=t_bad),
               dict(tq=changed(time_q, 0, 1)), dict(tq=changed(time_q, 9, time_q[8] - 1)), dict(tq=changed(time_q, n - 1, 1 << 61)),
               dict(wq=changed(w_q, 4, -1)), dict(wq=changed(w_q, 4, (1 << 61) + 1))):
        assert ticks(**kw) == 1, kw
    # more than 2^31 ticks: WA_ERR_CAPACITY, the handle is NULL, nothing else is written
    assert ticks(tq=changed(time_q, n - 1, 1 << 60), tick=2.0 ** -30, expect_handle=None) == 7
    for h in (t, t_bad, t_huge):
        h.close()


def test_plan_batch_tick_poses():
    """examples/plan_batch.py with --tick-poses ends with the tick_poses report; the run without the flag prints what it printed"""
    base = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py"), "--grid", "32", "--points", "6", "--exact-paths", "--shortcut", "--fit",
            "--retime", "--torch", "16"]
    a = subprocess.run(base + ["--tick-poses", "2.0"], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stdout[-800:] + a.stderr[-2000:]
    ra = json.loads(a.stdout.strip().splitlines()[-1])
    tp = ra["tick_poses"]
    assert tp["omega"] == 2.0 and tp["smooth"]["n"] == tp["limits"]["n"] and tp["ticks"]["n_ticks"] > 1
    assert tp["duration_turn_limited"] >= tp["duration_free"] > 0 and tp["max_tick_turn"] == tp["ticks"]["max_tick_turn"]
    assert tp["blocked_ticks"] == tp["ticks"]["n_blocked"]
    b = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-800:] + b.stderr[-2000:]
    rb = json.loads(b.stdout.strip().splitlines()[-1])
    assert "tick_poses" not in rb
    def results(d):   # everything but the wall-clock figures and the new report
        if isinstance(d, dict):
            return {k: results(v) for k, v in d.items() if not (k.startswith("t_") or k.endswith("_per_s") or k == "tick_poses")}
        return d
    assert results(ra) == results(rb)
