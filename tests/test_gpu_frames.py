"""GPU tests of wa_traj_retime_jerk_frames through the C ABI against tests/frames_ref.py (rules 61 - 67 of the header in numpy), bit for
bit: the laterals and the woven positions read back from the device, the axes, blocked, all five summaries; without a weave also
against a plain wa_traj_retime_jerk_axes call on the same arguments.

The tick kernel takes 256 ticks per workgroup and 64 per wavefront.  Every pointed case first asserts ON THE RESTATEMENT'S OUTPUT that
the scene does what it is for, and only then goes to the device.  (No case above 2^31 ticks: the capacity path is jerk_run's and
tests/test_gpu_jerk_axes.py covers it.)"""
import ctypes as C

import numpy as np
import pytest

import frames_ref as F
import jerk_axes_ref as X
import retime_ref as R
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG = 1
LIM = R.limits(v_max=4.0, acc=8.0, dec=8.0)
T = X.T
UP, DOWN, ALONG, ZED = np.array([0, 16384, 0]), np.array([0, -16384, 0]), np.array([16384, 0, 0]), np.array([0, 0, 16384])
TRI = F.triangle(16)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


@pytest.fixture(scope="module")
def wall16(ctx):
    """a 16^3 grid whose metal is the wall x = 8, y < 9: (restatement's grid, device grid)"""
    grid = X.wall_grid(16)
    g = grid_of(ctx, grid)
    yield grid, g
    g.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(ctx, c, W, g, weave="case", plain=False):
    """the library on a case: retime_jerk_frames' tuple with the three trajectories read back (retime_jerk_axes' with plain=True)"""
    t = api.Trajectory.from_points(ctx, c["xyz"])
    lim = c["lim"]
    kw = dict(dwell=c.get("dwell"), seg_tag=c.get("tag"), a_lat=lim["a_lat"], grid=g, v_near=lim["v_near"], near_d2=lim["near_d2"], s_q=True,
              tool=c.get("tool") if g is not None else None, near_add=c.get("near_add", -1))
    weave = c.get("weave") if isinstance(weave, str) else weave
    try:
        if plain:
            out = list(t.retime_jerk_axes(c["q"], lim["v_max"], lim["acc"], lim["dec"], c["tick"], W, **kw))
        else:
            out = list(t.retime_jerk_frames(c["q"], lim["v_max"], lim["acc"], lim["dec"], c["tick"], W, weave=weave, **kw))
        for k in (3, 9, 12):
            if k < len(out) and out[k] is not None:
                h = out[k]
                out[k] = h.points()
                h.close()
        return out
    finally:
        t.close()


def restate(c, W, grid=None, weave="case"):
    return F.retime_jerk_frames(c["xyz"], c["q"], c["lim"], c.get("dwell"), W, None, grid, c.get("tool") if grid is not None else None,
                                c.get("near_add", -1), c["tick"], c.get("tag"), c.get("weave") if isinstance(weave, str) else weave)


def same(ctx, c, W, grid=None, g=None, weave="case", r=None):
    """one call against the restatement: everything it returns; without a weave also against the plain call"""
    weave = c.get("weave") if isinstance(weave, str) else weave
    r = restate(c, W, grid, weave) if r is None else r
    out = call(ctx, c, W, g, weave)
    time_q, w_q, bound, pts, s_q, tags, s, ss, sj, axes, blocked, sa, lat, sf = out
    what = (len(c["xyz"]), W, c["tick"], grid is not None, sf, sa)
    assert sf == r["frames_summary"], (what, r["frames_summary"])
    assert sa == r["axes_summary"], (what, r["axes_summary"])
    assert s == r["summary"] and ss == r["stops"] and sj == r["jerk"], (what, s, ss, sj)
    assert np.array_equal(bits(lat), bits(r["lat"])), (what, np.flatnonzero((bits(lat) != bits(r["lat"])).any(1))[:5])
    assert np.array_equal(bits(pts), bits(r["ticks"])), (what, np.flatnonzero((bits(pts) != bits(r["ticks"])).any(1))[:5])
    assert np.array_equal(bits(axes), bits(r["axes"])), what
    assert np.array_equal(blocked, r["blocked"]), (what, np.flatnonzero(blocked != r["blocked"])[:5])
    assert np.array_equal(w_q, r["w_q"]) and np.array_equal(time_q, r["time_q"]) and np.array_equal(bound, r["bound"]), what
    assert np.array_equal(s_q, r["s_q"]), what
    assert (tags is None and r["tag"] is None) or np.array_equal(tags, r["tag"]), what
    if weave is None:
        plain = call(ctx, c, W, g, plain=True)
        for a, b in zip(out[:12], plain):
            assert (a is None and b is None) or (np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b), what
        assert bits(out[3]).tobytes() == bits(plain[3]).tobytes() and bits(out[9]).tobytes() == bits(plain[9]).tobytes()
    return r, out


# ------------------------------------------------------------------ seeded random cases
@pytest.mark.parametrize("seed", range(12))
def test_random_cases(ctx, seed):
    c = F.random_case(seed)
    g = grid_of(ctx, c["grid"])
    try:
        for W in (1, 2, 3, 7, 64, 300):
            same(ctx, c, W, c["grid"], g)
        same(ctx, c, [1, 7, 64][seed % 3], c["grid"], g, weave=None)
    finally:
        g.close()


# ------------------------------------------------------------------ pointed cases
def line_case(length, per=12, y=12.0, tick=0.01, q0=ZED, q1=ZED, x0=2.0, weave=None, tag=None):
    """a straight pass along +x from x0 at height y, z = 8, the axis turning evenly from q0 to q1 (both +z: the lateral is +y)"""
    xyz = R.densify([[x0, y, 8], [x0 + length, y, 8]], per)
    w = np.linspace(0.0, 1.0, len(xyz))[:, None]
    return dict(xyz=xyz, q=T.quantise_all(q0 * (1 - w) + q1 * w), lim=LIM, tick=tick, tool=T.rod(3, 16 * 5, 1), near_add=2,
                tag=np.ones(len(xyz) - 1, np.uint8) if tag is None else np.asarray(tag, np.uint8),
                weave=F.weave(0.25, 0.75, TRI, 0.125) if weave is None else weave)


@pytest.mark.parametrize("target", [63, 64, 65, 255, 256, 257])
def test_tick_counts_across_wavefronts_and_workgroups(ctx, wall16, target):
    c = line_case(2.0, tick=0.05 if target < 100 else (0.02 if target < 200 else 0.01), q1=UP)
    n_u = X.J.retime_jerk(c["xyz"], c["lim"], None, 1, tick=c["tick"], want_ticks=False)["jerk"]["n_in"]
    W = target - n_u + 1
    assert 1 <= W < 200, (n_u, W)
    r = restate(c, W, wall16[0])
    assert r["frames_summary"]["n_ticks"] == target and r["frames_summary"]["n_no_lateral"] == 0 and r["moved"].sum() > target // 2
    assert r["frames_summary"]["max_lat_turn"] > 0
    same(ctx, c, W, *wall16, r=r)


def dense_line(tag_of=None, **kw):
    """6 units at 4 per second in ticks of 5 ms: about 400 ticks, 0.02 per tick at full speed, on segments of 1 / 150"""
    c = line_case(6.0, per=900, tick=0.005, **kw)
    r0 = restate(c, 1, weave=None)
    if tag_of is not None:
        c["tag"] = tag_of(r0)
    return c, r0


def test_a_run_inside_one_wavefront(ctx, wall16):
    def tags(r0):
        tag = np.zeros(900, np.uint8)
        tag[r0["seg"][70]:r0["seg"][120] + 1] = 1
        return tag

    c, _ = dense_line(tags)
    r = restate(c, 1, wall16[0])
    k = np.flatnonzero(r["weaving"])
    assert k[0] == 70 and k[-1] == 120 and k[0] // 64 == k[-1] // 64 and r["frames_summary"]["n_weave_runs"] == 1 and r["moved"][k[1:-1]].any()
    same(ctx, c, 1, *wall16, r=r)


def test_run_boundaries_on_tick_64_and_tick_256(ctx, wall16):
    def tags(r0):
        assert r0["seg"][63] < r0["seg"][64] and r0["seg"][255] < r0["seg"][256]
        tag = np.zeros(900, np.uint8)
        tag[r0["seg"][64]:r0["seg"][255] + 1] = 1
        return tag

    c, _ = dense_line(tags, weave=F.weave(0.25, 0.75, TRI, 0.0))
    r = restate(c, 1, wall16[0])
    w = r["weaving"]
    assert not w[63] and w[64] and w[255] and not w[256] and w.sum() == 192 and r["off_q"][255] != 0
    assert r["frames_summary"]["max_offset_step_q"] >= abs(int(r["off_q"][255]))   # (the step back to 0 on tick 256 counts)
    same(ctx, c, 1, *wall16, r=r)


def test_a_wavelength_shorter_than_one_ticks_travel(ctx, wall16):
    c = line_case(3.0, weave=F.weave(0.25, 0.003, TRI, 0.0))
    r = restate(c, 2, wall16[0])
    assert np.diff(r["s_q"]).max() > 2 * int(np.rint(0.003 * F.QF)) and len(set(r["off_q"].tolist())) > 20
    same(ctx, c, 2, *wall16, r=r)


def test_a_pattern_of_two_entries(ctx, wall16):
    c = line_case(3.0, weave=F.weave(0.25, 0.5, [0, 16384], 0.0))
    r = restate(c, 3, wall16[0])
    assert r["off_q"].min() == 0 and r["off_q"].max() > int(0.2 * F.QF)
    same(ctx, c, 3, *wall16, r=r)


def test_a_taper_longer_than_half_the_run_and_no_taper(ctx, wall16):
    c = line_case(3.0, weave=F.weave(0.5, 0.25, TRI, 2.0))
    r = restate(c, 2, wall16[0])
    assert 0 < r["frames_summary"]["max_offset_q"] < int(0.5 * F.QF * 0.76) and r["off_q"][0] == 0 and r["off_q"][-1] == 0   # (env <= 1.5 / 2)
    same(ctx, c, 2, *wall16, r=r)
    c = line_case(3.0, weave=F.weave(0.5, 0.25, TRI, 0.0))
    r = restate(c, 2, wall16[0])
    assert r["frames_summary"]["max_offset_q"] > int(0.5 * F.QF * 0.9)
    same(ctx, c, 2, *wall16, r=r)


def test_a_torch_along_the_travel_direction_has_no_lateral(ctx, wall16):
    c = line_case(3.0, q0=ALONG, q1=ALONG)
    r = restate(c, 2, wall16[0])
    s = r["frames_summary"]
    assert s["n_no_lateral"] == s["n_ticks"] == s["n_weave_ticks"] and s["max_offset_q"] > 0 and not r["moved"].any() and s["max_lat_turn"] == 0
    assert r["ticks"].tobytes() == r["base_ticks"].tobytes() and not r["lat"].any()
    same(ctx, c, 2, *wall16, r=r)


def test_a_path_that_doubles_back_exactly(ctx, wall16):
    a = R.densify([[2, 12, 8], [5, 12, 8]], 4)
    xyz = np.concatenate([a, a[-2::-1]]).astype(np.float32)
    n = len(xyz)
    c = dict(xyz=xyz, q=np.tile(ZED, (n, 1)), lim=LIM, tick=0.01, tool=T.rod(3, 16 * 5, 1), near_add=2, tag=np.ones(n - 1, np.uint8),
             weave=F.weave(0.25, 0.75, TRI, 0.125))
    r = restate(c, 1, wall16[0])
    assert (r["tau"][len(a) - 1] == 0).all() and (r["tau"][len(a) - 2] == ALONG).all() and (r["tau"][len(a)] == -ALONG).all()
    assert (r["ql"][:, 1] > 0).any() and (r["ql"][:, 1] < 0).any() and r["frames_summary"]["max_lat_turn"] >= (1 << 20) - 1
    same(ctx, c, 1, *wall16, r=r)
    same(ctx, c, 6, *wall16)


def test_coincident_samples_at_both_ends_and_a_turning_stop_inside_the_run(ctx, wall16):
    a = R.densify([[2, 12, 8], [5, 12, 8]], 7)
    b = R.densify([[5, 12, 8], [5, 14, 8]], 5)
    xyz, dw = X.polyline([(a[:1], []), (a, [0.05, -1.0]), (b, [0.2]), (b[-1:], [-1.0, 0.08])])
    n = len(xyz)
    q = np.tile(X.fixed_axis((0.0, -1.0, 1.0)), (n, 1))
    q[len(a) + 2:] = X.fixed_axis((1.0, 0.0, 1.0))
    c = dict(xyz=xyz, q=q, dwell=dw, lim=LIM, tick=0.01, tool=T.rod(2, 48, 0), near_add=1, tag=np.ones(n - 1, np.uint8),
             weave=F.weave(0.25, 0.8125, TRI, 0.25))
    for W in (1, 5):
        r = restate(c, W, wall16[0])
        s = r["frames_summary"]
        assert r["rest"][0] and r["rest"][-1] and (r["tau"][:3] == ALONG).all() and (r["tau"][-3:] == UP).all() and s["n_no_lateral"] == 0
        mid = np.flatnonzero(r["rest"] & (r["seg"] == len(a) + 1))
        assert len(mid) >= 20 and len(set(r["off_q"][mid].tolist())) == 1 and r["off_q"][mid[0]] != 0 and s["n_weave_runs"] == 1
        assert len({tuple(v) for v in r["ql"][mid].tolist()}) > 10 and r["axes_summary"]["n_turning_rests"] >= 1
        same(ctx, c, W, *wall16, r=r)


def test_two_runs_separated_by_one_segment(ctx, wall16):
    tag = np.ones(12, np.uint8)
    tag[5] = 0
    c = line_case(3.0, tag=tag)
    r = restate(c, 2, wall16[0])
    w = r["weaving"]
    assert r["frames_summary"]["n_weave_runs"] == 2 and w[0] and w[-1] and 5 < (~w).sum() < w.sum()
    gap = np.flatnonzero(~w)
    assert r["off_q"][gap[0] - 3] != 0 and r["off_q"][gap[-1] + 3] != 0 and abs(int(r["off_q"][gap[0] - 1])) < int(0.1 * F.QF)   # (tapered)
    same(ctx, c, 2, *wall16, r=r)


def test_a_weave_into_the_wall_and_a_weave_out_of_the_grid(ctx, wall16):
    """the pass crosses the wall's plane x = 8 two voxels above its upper edge y = 8 (clear); a weave of 2.5 across the seam dips
    into the wall.  A second pass along y = 14.5 leaves the grid (y > 15) at every crest"""
    tool = T.rod(2, 16, 0)
    c = dict(line_case(10.0, y=10.5, x0=3.0, weave=F.weave(2.5, 0.4375, TRI, 0.0)), tool=tool)
    base = restate(c, 2, wall16[0], weave=None)
    r = restate(c, 2, wall16[0])
    assert base["axes_summary"]["n_blocked"] == 0 and base["axes_summary"]["first_blocked"] == -1 and base["axes_summary"]["n_outside"] == 0
    assert r["frames_summary"]["n_weave_blocked"] == r["axes_summary"]["n_blocked"] > 0 and r["axes_summary"]["first_blocked"] > 0
    same(ctx, c, 2, *wall16, r=r)
    c = line_case(10.0, y=14.5, x0=3.0, weave=F.weave(1.0, 0.4375, TRI, 0.0))
    base = restate(c, 2, wall16[0], weave=None)
    r = restate(c, 2, wall16[0])
    assert base["axes_summary"]["n_outside"] == 0 and 0 < r["axes_summary"]["n_outside"] < r["axes_summary"]["n_ticks"]
    same(ctx, c, 2, *wall16, r=r)


def test_without_a_grid_and_a_tool_and_without_a_weave(ctx, wall16):
    c = line_case(3.0, q1=UP)
    r, out = same(ctx, c, 6)
    assert not out[10].any() and r["axes_summary"]["n_outside"] == 0 and r["moved"].any()
    same(ctx, c, 6, weave=None)
    same(ctx, c, 6, *wall16, weave=None)
    same(ctx, c, 6, *wall16, weave=dict(c["weave"], amplitude=0.0))
    same(ctx, c, 6, *wall16, weave=dict(c["weave"], tag_mask=2, tag_value=2))
    same(ctx, dict(c, tag=None), 6, *wall16, weave=None)


def test_the_same_bytes_twice(ctx):
    c = F.random_case(4)
    g = grid_of(ctx, c["grid"])
    try:
        a, b = call(ctx, c, 7, g), call(ctx, c, 7, g)
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y)
        for k in (3, 9, 12):
            assert bits(a[k]).tobytes() == bits(b[k]).tobytes()
    finally:
        g.close()


def test_every_refusal_writes_nothing(ctx, wall16):
    c = line_case(3.0)
    n = len(c["xyz"])
    t = api.Trajectory.from_points(ctx, c["xyz"])
    g = wall16[1]
    q = np.ascontiguousarray(c["q"], np.int32)
    tool = api.torch_tool(*c["tool"])
    tag = np.ascontiguousarray(c["tag"], np.uint8)
    good = dict(amplitude=0.25, wavelength=0.75, taper=0.125, pattern=TRI, tag_mask=1, tag_value=1)
    cases = [
        ("NULL frames summary", dict(frames=False), {}),
        ("a weave without seg_tag", dict(tag=False), {}),
        ("a negative amplitude", {}, dict(amplitude=-0.25)),
        ("an infinite amplitude", {}, dict(amplitude=float("inf"))),
        ("a taper that is not a number", {}, dict(taper=float("nan"))),
        ("a negative taper", {}, dict(taper=-1.0)),
        ("an infinite wavelength", {}, dict(wavelength=float("inf"))),
        ("a wavelength that is not a number", {}, dict(wavelength=float("nan"))),
        ("wl_q = 0", {}, dict(wavelength=2.0 ** -32)),
        ("a negative wavelength", {}, dict(wavelength=-0.75)),
        ("wl_q above 2^50", {}, dict(wavelength=2.0 ** 20 + 1.0)),
        ("amp_q = 2^61", {}, dict(amplitude=2.0 ** 31)),
        ("taper_q = 2^61", {}, dict(taper=2.0 ** 31)),
        ("P = 1", {}, dict(pattern=[0])),
        ("P = 4097", {}, dict(pattern=[0] * 4097)),
        ("a NULL pattern", dict(pattern=False), {}),
        ("a pattern entry above 16384", {}, dict(pattern=[0, 5, 16385])),
        ("a pattern entry below -16384", {}, dict(pattern=[0, -16385])),
        ("pattern[0] != 0", {}, dict(pattern=[1, 0, 0])),
        ("tag_mask 0", {}, dict(tag_mask=0, tag_value=0)),
        ("NULL q (rule 56)", dict(q=False), {}),
        ("window 0 (rule 48)", dict(W=0), {}),
    ]
    try:
        for name, kw, change in cases:
            lim = L.RetimeLimits(4.0, 8.0, 8.0, float("inf"), 0.0, -1)
            w = api.make_weave(**dict(good, **change))
            if not kw.get("pattern", True):
                w.pattern = None
            poison = [np.full(n, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(n, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(n, 0x5A, np.uint8),
                      np.full(4096, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(4096, 0x5A, np.uint8), np.full(4096, 0x5A, np.uint8)]
            th, ah, lh = C.c_void_p(0x5A5A), C.c_void_p(0x5A5A), C.c_void_p(0x5A5A)
            sums = [L.RetimeSummary(), L.StopsSummary(), L.JerkSummary(), L.JerkAxesSummary(), L.FramesSummary()]
            for s in sums:
                C.memset(C.byref(s), 0x5A, C.sizeof(s))
            before = [bytes(s) for s in sums]
            has_tag = kw.get("tag", True)
            rc = ctx.lib.wa_traj_retime_jerk_frames(g.h, t.h, C.byref(lim), None, None, C.c_double(0.01), kw.get("W", 4),
                                                    tag.ctypes.data if has_tag else None, q.ctypes.data if kw.get("q", True) else None,
                                                    C.byref(tool), 2, C.byref(w), poison[0].ctypes.data, poison[1].ctypes.data,
                                                    poison[2].ctypes.data, C.byref(th), poison[3].ctypes.data,
                                                    poison[4].ctypes.data if has_tag else None, C.byref(ah), poison[5].ctypes.data, C.byref(lh),
                                                    C.byref(sums[0]), C.byref(sums[1]), C.byref(sums[2]), C.byref(sums[3]),
                                                    C.byref(sums[4]) if kw.get("frames", True) else None)
            assert rc == ARG, (name, rc)
            assert th.value == 0x5A5A and ah.value == 0x5A5A and lh.value == 0x5A5A, name
            assert all((p.view(np.uint8) == 0x5A).all() for p in poison), name
            assert [bytes(s) for s in sums] == before, name
        r, _ = same(ctx, c, 4, *wall16, weave=good)   # (the arguments the refusals were cut from are accepted)
        assert r["frames_summary"]["n_ticks"] <= 4096 and r["moved"].any()
    finally:
        t.close()
