"""GPU tests of wa_traj_retime_jerk_axes through the C ABI against tests/jerk_axes_ref.py (rules 56 - 60 of the header in numpy), bit for
bit: the axes read back from the device, blocked, all four summaries, and everything wa_traj_retime_jerk returns against a plain
wa_traj_retime_jerk call on the same arguments.

The tick kernel takes 256 ticks per workgroup and 64 per wavefront.  Every pointed case is built by a function that first asserts ON THE
RESTATEMENT'S OUTPUT that the scene does what it is for, and only then goes to the device.

One case of the list cannot be built: a short rest (n_short_rests > 0).  A stop's extended dwell lasts dq + (W - 1) tick_q, an interval
of that length holds at least floor(dq / tick_q) + W - 1 ticks k * tick_q, every one of them has U = GL_f (retime rule 6 finds the stop),
and a window of W such ticks averages to GL_f exactly: at least floor(dq / tick_q) rest ticks, always.  The counter stays in the
summaries compared below, where it is 0, as in every test of wa_traj_retime_jerk."""
import ctypes as C

import numpy as np
import pytest

import jerk_axes_ref as X
import retime_ref as R
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG, CAPACITY = 1, 7
LIM = R.limits(v_max=4.0, acc=8.0, dec=8.0)
T = X.T
UP, DOWN, ALONG = np.array([0, 16384, 0]), np.array([0, -16384, 0]), np.array([16384, 0, 0])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wall16(ctx):
    """a 16^3 grid whose metal is the wall x = 8, y < 9: (restatement's grid, device grid)"""
    grid = X.wall_grid(16)
    g = grid_of(ctx, grid)
    yield grid, g
    g.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(ctx, c, W, g, plain=False):
    """the library on a case: retime_jerk_axes's tuple with both trajectories read back (or retime_jerk's with plain=True)"""
    t = api.Trajectory.from_points(ctx, c["xyz"])
    lim = c["lim"]
    kw = dict(dwell=c.get("dwell"), seg_tag=c.get("tag"), a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"], s_q=True)
    try:
        if plain:
            out = list(t.retime_jerk(lim["v_max"], lim["acc"], lim["dec"], c["tick"], W, **kw))
        else:
            out = list(t.retime_jerk_axes(c["q"], lim["v_max"], lim["acc"], lim["dec"], c["tick"], W, tool=c.get("tool") if g is not None else None,
                                          near_add=c.get("near_add", -1), **kw))
        for k in (3, 9):
            if k < len(out) and out[k] is not None:
                h = out[k]
                out[k] = h.points()
                h.close()
        return out
    finally:
        t.close()


def same(ctx, c, W, grid=None, g=None):
    """one call against the restatement and against the plain call: everything it returns"""
    r = c.get("r")
    if r is None or r["jerk"]["window"] != W:
        r = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c.get("dwell"), W, None, grid, c.get("tool") if grid is not None else None,
                               c.get("near_add", -1), c["tick"], c.get("tag"))
    out = call(ctx, c, W, g)
    time_q, w_q, bound, pts, s_q, tags, s, ss, sj, axes, blocked, sa = out
    what = (len(c["xyz"]), W, c["tick"], grid is not None, sa)
    assert sa == r["axes_summary"], (what, r["axes_summary"])
    assert s == r["summary"] and ss == r["stops"] and sj == r["jerk"], (what, s, ss, sj)
    assert np.array_equal(bits(axes), bits(r["axes"])), (what, np.flatnonzero((bits(axes) != bits(r["axes"])).any(1))[:5])
    assert np.array_equal(blocked, r["blocked"]), (what, np.flatnonzero(blocked != r["blocked"])[:5])
    assert np.array_equal(w_q, r["w_q"]) and np.array_equal(time_q, r["time_q"]) and np.array_equal(bound, r["bound"]), what
    assert np.array_equal(s_q, r["s_q"]) and np.array_equal(bits(pts), bits(r["ticks"])), what
    assert (tags is None and r["tag"] is None) or np.array_equal(tags, r["tag"]), what
    plain = call(ctx, c, W, g, plain=True)
    for a, b in zip(out[:9], plain):
        assert (a is None and b is None) or (np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b), what
    return r, out


# ------------------------------------------------------------------ seeded random cases
@pytest.mark.parametrize("seed", range(12))
def test_random_cases(ctx, seed):
    c = X.random_case(seed)
    g = grid_of(ctx, c["grid"])
    try:
        n_u = X.J.retime_jerk(c["xyz"], c["lim"], c["dwell"], 1, None, c["grid"], c["tick"], want_ticks=False)["jerk"]["n_in"]
        for W in (1, 2, 3, 7, 64, 300) + ((n_u + 3,) if seed == 1 else ()):   # (seed 1: 397 ticks, a window longer than all of them)
            same(ctx, c, W, c["grid"], g)
    finally:
        g.close()


# ------------------------------------------------------------------ pointed cases
def line_case(length, per=12, y=12.0, tick=0.01, q0=UP, q1=ALONG):
    """a straight pass along x from x = 2 at height y, z = 8, the axis turning evenly from q0 to q1"""
    xyz = R.densify([[2, y, 8], [2 + length, y, 8]], per)
    w = np.linspace(0.0, 1.0, len(xyz))[:, None]
    return dict(xyz=xyz, q=T.quantise_all(q0 * (1 - w) + q1 * w), lim=LIM, tick=tick, tool=T.rod(3, 16 * 5, 1), near_add=2,
                tag=(np.arange(len(xyz) - 1) + 1).astype(np.uint8))


def stop_case(before, after, dwell, q_a, q_e, tick=0.01, joint=None, y=12.0, x0=2.0, tool=None):
    """two straight pieces along x joined by a stop (joint: the dwells of the segments without length at the joint); the axis is q_a up
    to the joint's first sample and q_e from its last one on, and in a longer joint the samples between alternate q_e, q_a"""
    a = R.densify([[x0, y, 8], [x0 + before, y, 8]], 6)
    b = R.densify([[x0 + before, y, 8], [x0 + before + after, y, 8]], 5)
    joint = [dwell] if joint is None else joint
    xyz, dw = X.polyline([(a, []), (b, joint)])
    q = np.empty((len(xyz), 3), np.int64)
    q[:len(a)] = q_a
    q[len(a) + len(joint) - 1:] = q_e
    for j in range(len(joint) - 1):
        q[len(a) + j] = q_e if j % 2 == 0 else q_a
    return dict(xyz=xyz, q=q, dwell=dw, lim=LIM, tick=tick, tool=T.rod(3, 16 * 5, 0) if tool is None else tool, near_add=2,
                tag=(np.arange(len(xyz) - 1) + 1).astype(np.uint8), head=len(a) - 1 + [d >= 0 for d in joint].index(True))


def restate(c, W, grid=None):
    c["r"] = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c.get("dwell"), W, None, grid, c.get("tool") if grid is not None else None,
                                c.get("near_add", -1), c["tick"], c.get("tag"))
    return c["r"]


@pytest.mark.parametrize("target", [63, 64, 65, 255, 256, 257, 130])
def test_tick_counts_across_wavefronts_and_workgroups(ctx, wall16, target):
    """one cap everywhere: lowering changes nothing, n_u does not depend on W and W places n_ticks (130 is no multiple of 4)"""
    c = line_case(2.0, tick=0.05 if target < 100 else (0.02 if target < 200 else 0.01))
    n_u = X.J.retime_jerk(c["xyz"], c["lim"], None, 1, tick=c["tick"], want_ticks=False)["jerk"]["n_in"]
    W = target - n_u + 1
    assert 1 <= W < 200, (n_u, W)
    r = restate(c, W, wall16[0])
    assert r["axes_summary"]["n_ticks"] == target and len(np.unique(r["qt"], axis=0)) > 10
    assert r["s_q"][-1] >= r["GL"][r["seg"][-1] + 1] and np.array_equal(r["qt"][-1], X.K.quantise_rows(c["q"][-1:].astype(float))[0])   # p_(i+1) exactly
    same(ctx, c, W, *wall16)


@pytest.mark.parametrize("boundary,before,dwell", [(64, 0.4, 0.3), (256, 7.2, 0.4)])
def test_a_rest_across_a_wavefront_and_a_workgroup_boundary(ctx, wall16, boundary, before, dwell):
    c = stop_case(before, 1.0, dwell, UP, T.quantise_all([[1, -1, 0.3]])[0])
    r = restate(c, 4, wall16[0])
    k = np.flatnonzero(r["rest"])
    assert k[0] < boundary - 3 and k[-1] > boundary + 3 and (np.diff(k) == 1).all(), (k[0], k[-1])
    assert r["axes_summary"]["n_turning_rests"] == 1 and r["axes_summary"]["min_turn_ticks"] == len(k)
    assert len(np.unique(r["qt"][k], axis=0)) == len(k)   # (the torch turns at every rest tick)
    same(ctx, c, 4, *wall16)


def test_a_rest_of_exactly_one_tick(ctx, wall16):
    c = stop_case(1.0, 1.0, 0.004, UP, DOWN)
    r = restate(c, 1, wall16[0])
    assert r["rest"].sum() == 1 and r["lam"][r["rest"]][0] == 0.0 and np.array_equal(r["qt"][r["rest"]][0], UP)
    same(ctx, c, 1, *wall16)


def test_stops_on_the_first_and_the_last_segment(ctx, wall16):
    a = R.densify([[2, 12, 8], [5, 12, 8]], 7)
    xyz, dw = X.polyline([(a[:1], []), (a, [0.05]), (a[-1:], [0.08])])
    q = np.tile(ALONG, (len(xyz), 1))
    q[0], q[-1] = UP, DOWN
    c = dict(xyz=xyz, q=q, dwell=dw, lim=LIM, tick=0.01, tool=T.rod(2, 48, 0), near_add=1, tag=(np.arange(len(xyz) - 1) + 1).astype(np.uint8))
    assert dw[0] >= 0 and dw[-1] >= 0 and (dw[1:-1] < 0).all()
    for W in (1, 5):
        r = restate(c, W, wall16[0])
        assert r["rest"][0] and r["rest"][-1] and set(r["seg"][r["rest"]]) == {0, len(xyz) - 2} and r["axes_summary"]["n_turning_rests"] == 2
        assert np.array_equal(r["qt"][0], UP)
        same(ctx, c, W, *wall16)


def test_two_stops_in_a_row_and_segments_without_length_round_a_stop(ctx, wall16):
    """joint [0.05, 0.07]: two stops in a row act as one.  joint [-1, 0.06, -1]: an un-stopped segment without length directly in front
    of and directly behind the stop, so a < f and e > f + 1, and the samples between carry other axes that the turn passes over"""
    c = stop_case(1.5, 1.0, None, UP, ALONG, joint=[0.05, 0.07])
    r = restate(c, 3, wall16[0])
    f = c["head"]
    assert (r["seg"][r["rest"]] == f).all() and r["R"][f] >= 12 + 0 and r["axes_summary"]["n_turning_rests"] == 1
    same(ctx, c, 3, *wall16)
    c = stop_case(1.5, 1.0, None, UP, ALONG, joint=[-1.0, 0.06, -1.0])
    r = restate(c, 3, wall16[0])
    f = c["head"]
    a, e = X.runs(r["GL"], f)
    assert a == f - 1 and e == f + 2 and (r["seg"][r["rest"]] == f).all()
    k = np.flatnonzero(r["rest"])
    assert np.array_equal(r["qt"][k[0]], UP) and np.array_equal(r["qt"][k[0] - 1], UP) and np.array_equal(r["qt"][k[-1] + 1], ALONG)
    assert not np.array_equal(c["q"][f], UP) and not np.array_equal(c["q"][f + 1], ALONG)   # (the samples inside the run are passed over)
    same(ctx, c, 3, *wall16)


def test_an_antipodal_turn_takes_the_all_zero_branch_at_its_middle(ctx, wall16):
    c = stop_case(1.0, 1.0, 0.1, UP, DOWN)
    r = restate(c, 2, wall16[0])
    k = np.flatnonzero(r["rest"])
    assert len(k) % 2 == 0 and r["lam"][k[len(k) // 2]] == 0.5 and r["zero"][k[len(k) // 2]] and r["zero"].sum() == 1
    assert np.array_equal(r["qt"][k[len(k) // 2]], UP) and np.array_equal(r["qt"][k[len(k) // 2 + 1]], DOWN)
    same(ctx, c, 2, *wall16)


def test_without_a_grid_and_a_tool(ctx):
    c = stop_case(1.0, 1.0, 0.1, UP, ALONG)
    r, out = same(ctx, c, 6)
    assert not out[10].any() and r["axes_summary"]["n_outside"] == 0 and r["axes_summary"]["n_blocked"] == 0


def test_a_blocked_tick_inside_a_rest_first_in_the_last_partial_workgroup(ctx, wall16):
    """the pass runs two voxels above the wall's upper edge and stops right over it; at the stop the torch turns from along the pass to
    straight down, into the wall: the first blocked tick is a rest tick"""
    c = stop_case(6.0, 1.0, 0.2, ALONG, DOWN, tick=0.006, y=10.0, tool=T.rod(4, 16 * 4, 0))
    r = restate(c, 4, wall16[0])
    s = r["axes_summary"]
    assert s["n_ticks"] % 256 and s["first_blocked"] >= 256 * ((s["n_ticks"] - 1) // 256) > 0, s
    assert r["rest"][s["first_blocked"]] and not r["rest"][r["blocked"] != 0].all() and s["n_near"] > 0, s
    same(ctx, c, 4, *wall16)


def test_ticks_outside_the_grid(ctx, wall16):
    c = line_case(16.0, y=14.0, tick=0.02)
    r = restate(c, 5, wall16[0])
    assert 0 < r["axes_summary"]["n_outside"] < r["axes_summary"]["n_ticks"]
    same(ctx, c, 5, *wall16)


def test_the_same_bytes_twice(ctx, wall16):
    c = X.random_case(4)
    g = grid_of(ctx, c["grid"])
    try:
        a, b = call(ctx, c, 7, g), call(ctx, c, 7, g)
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y)
        assert bits(a[9]).tobytes() == bits(b[9]).tobytes() and a[10].tobytes() == b[10].tobytes()
    finally:
        g.close()


def test_more_than_two_to_the_31_ticks(ctx):
    c = line_case(10.0, tick=2.0 ** -30)   # (3 s at 2^30 ticks per second)
    r = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], None, 3, tick=c["tick"])
    assert r["axes"] is None and r["jerk"]["n_ticks"] > 1 << 31
    out = call(ctx, c, 3, None)
    assert out[3] is None and out[9] is None and out[10] is None and out[11] == r["axes_summary"] == dict.fromkeys(X.AXES_FIELDS, 0)
    assert out[6] == r["summary"] and out[8] == r["jerk"] and np.array_equal(out[0], r["time_q"])
    # ... and straight through the ABI: the status, *axes_out = NULL, blocked_out untouched
    t = api.Trajectory.from_points(ctx, c["xyz"])
    try:
        lim = L.RetimeLimits(4.0, 8.0, 8.0, float("inf"), 0.0, -1)
        q = np.ascontiguousarray(c["q"], np.int32)
        blocked = np.full(16, 0xA5, np.uint8)
        ah = C.c_void_p(0x5A5A)
        s, s2, s3, s4 = L.RetimeSummary(), L.StopsSummary(), L.JerkSummary(), L.JerkAxesSummary()
        s4.n_ticks = 77
        rc = ctx.lib.wa_traj_retime_jerk_axes(None, t.h, C.byref(lim), None, None, C.c_double(c["tick"]), 3, None, q.ctypes.data, None, -1, None, None,
                                              None, None, None, None, C.byref(ah), blocked.ctypes.data, C.byref(s), C.byref(s2), C.byref(s3),
                                              C.byref(s4))
        assert rc == CAPACITY and ah.value is None and (blocked == 0xA5).all() and s4.n_ticks == 0 and s3.n_ticks == r["jerk"]["n_ticks"]
    finally:
        t.close()


def test_every_refusal_of_rule_56_writes_nothing(ctx, wall16):
    c = stop_case(1.0, 1.0, 0.1, UP, ALONG)
    n = len(c["xyz"])
    t = api.Trajectory.from_points(ctx, c["xyz"])
    g = wall16[1]
    good_q = np.ascontiguousarray(c["q"], np.int32)
    good_tool = api.torch_tool(*c["tool"])

    def tool_with(**kw):
        tl = api.torch_tool(*c["tool"])
        for k, (j, v) in kw.items():
            if k == "n_beads":
                tl.n_beads = v
            else:
                getattr(tl, k)[j] = v
        return tl

    def bad_q(i, v):
        q = good_q.copy()
        q[i] = v
        return q

    cases = [
        ("NULL q", dict(q=None)),
        ("NULL axes summary", dict(axes=False)),
        ("a grid alone", dict(tool=None)),
        ("a tool alone", dict(g=None)),
        ("a component above 16384", dict(q=bad_q(3, (16385, 0, 0)))),
        ("a component below -16384", dict(q=bad_q(n - 1, (0, -16385, 0)))),
        ("an all-zero axis", dict(q=bad_q(0, (0, 0, 0)))),
        ("no bead", dict(tool=tool_with(n_beads=(0, 0)))),
        ("65 beads", dict(tool=tool_with(n_beads=(0, 65)))),
        ("a negative dist16", dict(tool=tool_with(dist16=(1, -1)))),
        ("dist16 above 65536", dict(tool=tool_with(dist16=(0, 65537)))),
        ("a negative r2", dict(tool=tool_with(r2=(2, -1)))),
        ("r2 above 2^30", dict(tool=tool_with(r2=(0, (1 << 30) + 1)))),
        ("near_add above 2^30", dict(near_add=(1 << 30) + 1)),
        ("window 0 (rule 48)", dict(W=0)),
        ("NULL jerk summary (rule 48)", dict(jerk=False)),
        ("a stop on a segment that has a length (rule 40)", dict(dwell=np.where(np.arange(n - 1) == 1, 0.1, -1.0))),
    ]
    try:
        for name, kw in cases:
            lim = L.RetimeLimits(4.0, 8.0, 8.0, float("inf"), 0.0, -1)
            q = kw.get("q", good_q)
            tool = kw.get("tool", good_tool)
            gh = kw["g"] if "g" in kw else g
            dwell = np.ascontiguousarray(kw.get("dwell", c["dwell"]), np.float64)
            poison = [np.full(n, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(n, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(n, 0x5A, np.uint8),
                      np.full(4096, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(4096, 0x5A, np.uint8), np.full(4096, 0x5A, np.uint8)]
            th, ah = C.c_void_p(0x5A5A), C.c_void_p(0x5A5A)
            sums = [L.RetimeSummary(), L.StopsSummary(), L.JerkSummary(), L.JerkAxesSummary()]
            for s in sums:
                C.memset(C.byref(s), 0x5A, C.sizeof(s))
            before = [bytes(s) for s in sums]
            rc = ctx.lib.wa_traj_retime_jerk_axes(gh.h if gh is not None else None, t.h, C.byref(lim), None, dwell.ctypes.data, C.c_double(0.01),
                                                  kw.get("W", 4), None, q.ctypes.data if q is not None else None,
                                                  C.byref(tool) if tool is not None else None, kw.get("near_add", 2), poison[0].ctypes.data,
                                                  poison[1].ctypes.data, poison[2].ctypes.data, C.byref(th), poison[3].ctypes.data, None,
                                                  C.byref(ah), poison[5].ctypes.data, C.byref(sums[0]), C.byref(sums[1]),
                                                  C.byref(sums[2]) if kw.get("jerk", True) else None, C.byref(sums[3]) if kw.get("axes", True) else None)
            assert rc == ARG, (name, rc)
            assert th.value == 0x5A5A and ah.value == 0x5A5A, name
            assert all((p.view(np.uint8) == 0x5A).all() for p in poison), name
            assert [bytes(s) for s in sums] == before, name
        r, _ = same(ctx, c, 4, *wall16)   # (the arguments the refusals were cut from are accepted)
        assert r["axes_summary"]["n_ticks"] <= 4096
    finally:
        t.close()
