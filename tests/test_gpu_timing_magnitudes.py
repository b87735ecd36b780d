"""GPU tests of the timing calls (wa_traj_retime, wa_traj_retime_stops, wa_traj_retime_jerk, wa_traj_tick_axes, wa_traj_tick_axes_stops)
through the C ABI on the scenes of tests/magnitude_ref.py, bit for bit against the numpy restatements: long paths, prefix sums of U
that wrap modulo 2^64, caps saturated at 2^61 and caps of 0 and 1 quantum, sums and durations just under 2^61.  The other GPU files of
the family visit every scan tile and workgroup edge in the sample and tick counts at paths 1 - 5 units long; this one keeps the counts
small (third_level apart: the scans' third level together with the wrap) and leaves the small magnitudes.

tests/test_timing_magnitude_rules.py holds the restatements against Python integers on the same scenes; magnitude_ref.reference()
asserts every scene's regime wherever it is used.  Every refusal here is a cleanly refused argument set one step behind an accepted
one: nothing provokes a fault."""
import ctypes as C
import os

import numpy as np
import pytest

import jerk_ref as J
import magnitude_ref as M
import retime_ref as R
import stops_ref as S
import ticks_ref as K
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG = 1


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def summary_of(s):
    return {k: (list(getattr(s, k)) if k == "n_bound" else int(getattr(s, k))) for k, _ in type(s)._fields_}


def rows(a, b):
    """the first rows at which two arrays differ (for the message of a failed comparison)"""
    d = np.asarray(a) != np.asarray(b)
    return np.flatnonzero(d.any(1) if d.ndim > 1 else d)[:5]


def same_profile(what, got, r):
    """(time_q, w_q, bound, tick points, summary) of a call against a restatement's dictionary"""
    time_q, w_q, bound, pts, s = got
    assert s == r["summary"], (what, s, r["summary"])
    assert np.array_equal(w_q, r["w_q"]), (what, rows(w_q, r["w_q"]))
    assert np.array_equal(time_q, r["time_q"]), (what, rows(time_q, r["time_q"]))
    assert np.array_equal(bound, r["bound"]), (what, rows(bound, r["bound"]))
    assert pts.shape == r["ticks"].shape, (what, pts.shape, r["ticks"].shape)
    assert np.array_equal(bits(pts), bits(r["ticks"])), (what, rows(bits(pts), bits(r["ticks"])))


def same_jerk(what, got, r, tagged):
    """everything wa_traj_retime_jerk returns against jerk_ref.retime_jerk's dictionary"""
    time_q, w_q, bound, pts, s_q, tags, s, ss, sj = got
    assert ss == r["stops"], (what, ss, r["stops"])
    assert sj == r["jerk"], (what, sj, r["jerk"])
    same_profile(what, (time_q, w_q, bound, pts, s), r)
    assert np.array_equal(s_q, r["s_q"]), (what, rows(s_q, r["s_q"]))
    if tagged:
        assert np.array_equal(tags, r["tag"]), (what, rows(tags, r["tag"]))
    else:
        assert tags is None and r["tag"] is None


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert (x == y) if isinstance(x, dict) else (x is None and y is None) or np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def points_of(h):
    if h is None:
        return None
    p = h.points()
    h.close()
    return p


def run_jerk(ctx, name):
    xyz, lim, tick, W, dwell, v_limit, seg_tag = M.scene(name)
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        out = t.retime_jerk(lim["v_max"], lim["acc"], lim["dec"], tick, W, dwell=dwell, seg_tag=seg_tag, a_lat=lim["a_lat"], v_limit=v_limit,
                            s_q=True)
        return out[:3] + (points_of(out[3]),) + out[4:]
    finally:
        t.close()


FILL = dict(time_q=-7, w_q=-7, bound=77, s_q=-7, tag=77)


def fresh(struct):
    """a summary whose every byte is 0xf9: a refused call leaves it so"""
    s = struct()
    C.memset(C.byref(s), 0xf9, C.sizeof(s))
    return s


def untouched(s):
    return bytes(s) == b"\xf9" * C.sizeof(s)


def raw_jerk(ctx, t, lim, W, tick, dwell, v_limit, seg_tag, n, n_ticks, skip=()):
    """the C call itself on filled outputs: (rc, outputs, ticks handle, the three summaries)"""
    lm = L.RetimeLimits(lim["v_max"], lim["acc"], lim["dec"], lim["a_lat"], lim["v_near"], lim["near_d2"])
    o = dict(time_q=np.full(n, -7, np.int64), w_q=np.full(n, -7, np.int64), bound=np.full(n, 77, np.uint8), s_q=np.full(n_ticks, -7, np.int64),
             tag=np.full(n_ticks, 77, np.uint8))
    th, s, s2, s3 = C.c_void_p(4242), fresh(L.RetimeSummary), fresh(L.StopsSummary), fresh(L.JerkSummary)
    P = lambda k: None if k in skip or (k == "tag" and seg_tag is None) else o[k].ctypes.data
    A = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    dwell, v_limit, seg_tag = A(dwell, np.float64), A(v_limit, np.float32), A(seg_tag, np.uint8)
    D = lambda a: None if a is None else a.ctypes.data
    rc = ctx.lib.wa_traj_retime_jerk(None, t.h, C.byref(lm), D(v_limit), D(dwell), C.c_double(tick), W, D(seg_tag), P("time_q"), P("w_q"),
                                     P("bound"), None if "ticks" in skip else C.byref(th), P("s_q"), P("tag"), C.byref(s), C.byref(s2),
                                     C.byref(s3))
    return rc, o, th, (s, s2, s3)


def raw_profile(ctx, t, lim, tick, dwell, v_limit, n, stops):
    """wa_traj_retime (stops False) or wa_traj_retime_stops on filled outputs"""
    lm = L.RetimeLimits(lim["v_max"], lim["acc"], lim["dec"], lim["a_lat"], lim["v_near"], lim["near_d2"])
    o = dict(time_q=np.full(n, -7, np.int64), w_q=np.full(n, -7, np.int64), bound=np.full(n, 77, np.uint8))
    th, s, s2 = C.c_void_p(4242), fresh(L.RetimeSummary), fresh(L.StopsSummary)
    A = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    dwell, v_limit = A(dwell, np.float64), A(v_limit, np.float32)
    D = lambda a: None if a is None else a.ctypes.data
    if stops:
        rc = ctx.lib.wa_traj_retime_stops(None, t.h, C.byref(lm), D(v_limit), D(dwell), C.c_double(tick), D(o["time_q"]), D(o["w_q"]),
                                          D(o["bound"]), C.byref(th), C.byref(s), C.byref(s2))
    else:
        rc = ctx.lib.wa_traj_retime(None, t.h, C.byref(lm), D(v_limit), C.c_double(tick), D(o["time_q"]), D(o["w_q"]), D(o["bound"]), C.byref(th),
                                    C.byref(s))
    return rc, o, th, (s, s2)


def refused(what, rc, o, th, sums):
    """WA_ERR_ARG, every output still its fill pattern, the handle and the summaries untouched"""
    assert rc == ARG, (what, rc)
    for k in o:
        assert (o[k] == FILL[k]).all(), (what, k)
    assert th.value == 4242 and all(untouched(s) for s in sums), what


# ------------------------------------------------------------------ wa_traj_retime_jerk
@pytest.mark.parametrize("name", M.SMALL)
def test_retime_jerk(ctx, name):
    """the call on every scene, and once more with ticks_out and s_q_out NULL, each alone and both"""
    xyz, lim, tick, W, dwell, v_limit, seg_tag = M.scene(name)
    r = M.reference(name)
    same_jerk(name, run_jerk(ctx, name), r, seg_tag is not None)
    n, n_ticks = len(xyz), r["jerk"]["n_ticks"]
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        for skip in (("ticks",), ("s_q",), ("ticks", "s_q")):
            rc, o, th, (s, s2, s3) = raw_jerk(ctx, t, lim, W, tick, dwell, v_limit, seg_tag, n, n_ticks, skip)
            what = (name, skip)
            assert rc == 0 and summary_of(s) == r["summary"] and summary_of(s2) == r["stops"] and summary_of(s3) == r["jerk"], what
            for k in ("time_q", "w_q", "bound"):
                assert np.array_equal(o[k], r[k]), (what, k)
            assert (o["s_q"] == -7).all() if "s_q" in skip else np.array_equal(o["s_q"], r["s_q"]), what
            assert np.array_equal(o["tag"], r["tag"]) if seg_tag is not None else (o["tag"] == 77).all(), what
            if "ticks" in skip:
                assert th.value == 4242, what
            else:
                pts = points_of(api.Trajectory(ctx, th))
                assert np.array_equal(bits(pts), bits(r["ticks"])), (what, rows(bits(pts), bits(r["ticks"])))
    finally:
        t.close()


def test_third_scan_level_with_wrapped_sums(ctx):
    """more than 2^22 + 1 prefix sums (the scan's third level) that pass 2^64; beside test_gpu_jerk's four million ticks on a line of
    length 2, whose sums end at 2^52"""
    r = M.reference("third_level")
    same_jerk("third_level", run_jerk(ctx, "third_level"), r, False)


# ------------------------------------------------------------------ wa_traj_retime, wa_traj_retime_stops
@pytest.mark.parametrize("stops", [False, True])
@pytest.mark.parametrize("name", M.PROFILE_SCENES)
def test_retime_and_retime_stops(ctx, name, stops):
    xyz, lim, tick, _, dwell, v_limit, _ = M.scene(name)
    r = M.profile_reference(name, stops)
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        kw = dict(a_lat=lim["a_lat"], v_limit=v_limit)
        if stops:
            time_q, w_q, bound, ticks, s, ss = t.retime_stops(lim["v_max"], lim["acc"], lim["dec"], tick, dwell=dwell, **kw)
            assert ss == r["stops"], (name, ss, r["stops"])
        else:
            time_q, w_q, bound, ticks, s = t.retime(lim["v_max"], lim["acc"], lim["dec"], tick, **kw)
        same_profile((name, stops), (time_q, w_q, bound, points_of(ticks), s), r)
    finally:
        t.close()


# ------------------------------------------------------------------ wa_traj_tick_axes, wa_traj_tick_axes_stops
@pytest.mark.parametrize("name", M.AXES_SCENES)
def test_tick_axes_on_large_profiles(ctx, name):
    """the axes of ticks_ref.stepped_axes at the ticks of the scene's profile (the restatement's time_q and w_q, which the device's
    were held against above): times near 2^61, squared speeds of 2^61 and of one quantum"""
    xyz, lim, tick, _, dwell, v_limit, seg_tag = M.scene(name)
    n = len(xyz)
    q = K.stepped_axes(n)
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        # (wa_traj_tick_axes on a profile with dwells: rule 6 alone, the axis of a dwell's ticks is the stop's first one)
        for stops, call_stops in ((False, False), (True, True)) + (((True, False),) if dwell is not None else ()):
            p = M.profile_reference(name, stops)
            args = (q, p["time_q"], p["w_q"], lim["acc"], lim["dec"], tick)
            what = (name, stops, call_stops)
            if call_stops:
                r = S.tick_axes_stops(xyz, q, p["time_q"], p["w_q"], lim["acc"], lim["dec"], tick, seg_tag=seg_tag)
                axes, blocked, sm, tags, st = t.tick_axes_stops(*args, seg_tag=seg_tag)
                assert st == r["stops"], (what, st, r["stops"])
                assert (tags is None and r["tag"] is None) if seg_tag is None else np.array_equal(tags, r["tag"]), what
                assert (st["n_dwell_ticks"] > 0) == (stops and dwell is not None), what
            else:
                r = K.tick_axes(xyz, q, p["time_q"], p["w_q"], lim["acc"], lim["dec"], tick)
                axes, blocked, sm = t.tick_axes(*args)
            a = points_of(axes)
            assert sm == r["summary"] and sm["n_ticks"] == p["summary"]["n_ticks"], (what, sm, r["summary"])
            assert np.array_equal(bits(a), bits(r["axes"])), (what, rows(bits(a), bits(r["axes"])))
            assert np.array_equal(blocked, r["blocked"]), what
            assert np.array_equal(bits(r["pos"]), bits(p["ticks"])), what   # the positions behind the axes are retime's ticks
    finally:
        t.close()


# ------------------------------------------------------------------ one step apart: accepted and refused
def test_window_127_is_accepted_and_128_refused(ctx):
    xyz, lim, tick, W, _, _, _ = M.scene("wrap_w127")
    r = M.reference("wrap_w127")
    assert W == 127 and not M.accepted(lambda: J.retime_jerk(xyz, lim, None, 128, tick=tick, want_ticks=False))
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        rc, o, th, (s, s2, s3) = raw_jerk(ctx, t, lim, 127, tick, None, None, None, len(xyz), r["jerk"]["n_ticks"])
        assert rc == 0 and summary_of(s3) == r["jerk"] and np.array_equal(o["s_q"], r["s_q"]) and np.array_equal(o["w_q"], r["w_q"])
        assert np.array_equal(bits(points_of(api.Trajectory(ctx, th))), bits(r["ticks"]))
        refused("W = 128", *raw_jerk(ctx, t, lim, 128, tick, None, None, None, len(xyz), r["jerk"]["n_ticks"] + 1))
    finally:
        t.close()


@pytest.mark.parametrize("name", ["saturated_acc", "saturated_dec", "saturated_2049"])
def test_ramps_one_step_below_the_refusal(ctx, name):
    """acc (dec) = 2^20 * 0.999 is accepted by all three calls (the scenes' own tests hold its bytes); at 2^20 the sum of A (of D) is
    2^61 and all three refuse"""
    xyz, lim, tick, W, _, _, _ = M.scene(name)
    r = M.reference(name)
    n = len(xyz)
    over = dict(lim, **{k: 2.0 ** 20 for k in ("acc", "dec") if lim[k] == M.ACC_LAST})
    assert not M.accepted(lambda: R.retime(xyz, over, tick=tick, want_ticks=False))
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        rc, o, th, (s, _) = raw_profile(ctx, t, lim, tick, None, None, n, False)
        assert rc == 0 and np.array_equal(o["w_q"], M.profile_reference(name, False)["w_q"]) and th.value != 4242
        api.Trajectory(ctx, th).close()
        refused((name, "retime"), *raw_profile(ctx, t, over, tick, None, None, n, False))
        refused((name, "retime_stops"), *raw_profile(ctx, t, over, tick, None, None, n, True))
        refused((name, "retime_jerk"), *raw_jerk(ctx, t, over, W, tick, None, None, None, n, r["jerk"]["n_ticks"]))
    finally:
        t.close()


def test_the_longest_extended_dwell_and_the_first_refused_one(ctx):
    """two samples at one place: the duration is dq + (W - 1) * tick_q, whose last accepted value and the next double behind it come
    from the restatement"""
    xyz, lim, good, bad = M.extended_dwell_pair()
    W, tick = M.PAIR_W, M.PAIR_TICK
    r = J.retime_jerk(xyz, lim, good, W, tick=tick)
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        n_ticks = r["jerk"]["n_ticks"]
        rc, o, th, (s, s2, s3) = raw_jerk(ctx, t, lim, W, tick, good, None, None, 2, n_ticks)
        assert rc == 0 and (summary_of(s), summary_of(s2), summary_of(s3)) == (r["summary"], r["stops"], r["jerk"])
        assert all(np.array_equal(o[k], r[k]) for k in ("time_q", "w_q", "bound", "s_q"))
        assert np.array_equal(bits(points_of(api.Trajectory(ctx, th))), bits(r["ticks"]))
        refused("extended dwell", *raw_jerk(ctx, t, lim, W, tick, bad, None, None, 2, n_ticks))
    finally:
        t.close()


@pytest.mark.parametrize("W", [1, M.PAIR_W])
def test_the_longest_duration_and_the_first_refused_one(ctx, W):
    """a line with a stop in the middle whose dwell brings the DURATION to 2^61 while the dwell itself, extended, stays below"""
    xyz, lim, good, bad = M.duration_pair(W)
    tick, n = M.PAIR_TICK, len(xyz)
    r = J.retime_jerk(xyz, lim, good, W, tick=tick)
    t = api.Trajectory.from_points(ctx, xyz)
    try:
        n_ticks = r["jerk"]["n_ticks"]
        rc, o, th, (s, s2, s3) = raw_jerk(ctx, t, lim, W, tick, good, None, None, n, n_ticks)
        assert rc == 0 and (summary_of(s), summary_of(s2), summary_of(s3)) == (r["summary"], r["stops"], r["jerk"])
        assert all(np.array_equal(o[k], r[k]) for k in ("time_q", "w_q", "bound", "s_q"))
        assert np.array_equal(bits(points_of(api.Trajectory(ctx, th))), bits(r["ticks"]))
        refused(("duration", W), *raw_jerk(ctx, t, lim, W, tick, bad, None, None, n, n_ticks))
        if W == 1:
            p = S.retime_stops(xyz, lim, good, tick=tick)
            rc, o, th, (s, s2) = raw_profile(ctx, t, lim, tick, good, None, n, True)
            assert rc == 0 and (summary_of(s), summary_of(s2)) == (p["summary"], p["stops"])
            assert all(np.array_equal(o[k], p[k]) for k in ("time_q", "w_q", "bound"))
            assert np.array_equal(bits(points_of(api.Trajectory(ctx, th))), bits(p["ticks"]))
            refused("duration, retime_stops", *raw_profile(ctx, t, lim, tick, bad, None, n, True))
    finally:
        t.close()


# ------------------------------------------------------------------ the same bytes again, and in a hostile context
def test_two_calls_the_same_bytes(ctx):
    for name in ("wrap_w8", "wrap_w127", "stops_w4", "stops_w25"):
        M.reference(name)
        same_bytes(run_jerk(ctx, name), run_jerk(ctx, name))


def make_ctx(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_wrapped_sums_in_poisoned_and_guarded_scratch(ctx):
    """scene 1 in a context whose device blocks start out filled and lie between red zones: the bytes of the restatement, no stray
    write, and behind a trim the live blocks of a fresh guarded context"""
    c = make_ctx(WA_DEV_POISON=1, WA_DEV_GUARD=1)
    try:
        c.trim()
        fresh_stats = c.guard_stats()
        for name in ("wrap_w1", "wrap_w8", "wrap_w127"):
            hostile = run_jerk(c, name)
            same_jerk(name, hostile, M.reference(name), False)
            same_bytes(run_jerk(ctx, name), hostile)
        assert c.poison_stats()["plain_blocks"] > 0
        c.trim()
        s = c.guard_stats()
        assert s["front_damaged"] + s["back_damaged"] == 0 and s["checked"] > 0, s
        assert s["live_blocks"] == fresh_stats["live_blocks"] and s["live_bytes"] == fresh_stats["live_bytes"], (fresh_stats, s)
    finally:
        c.close()
