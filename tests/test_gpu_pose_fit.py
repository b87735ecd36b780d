"""GPU tests of wa_grid_pose_fit_trajectory through the C ABI against tests/pose_fit_ref.py (rules 37 - 39 of the torch section in numpy),
bit for bit: knots, control points, samples, levels, the direction and the blocked byte of every segment, every field of the summary.
tests/test_pose_fit_rules.py checks the restatement itself and records the scenes' figures.

Sizes: k_pfit_segments gives one lane to a segment, 64 to a wavefront, 256 to a workgroup (9, 64, 65, 257 and 2 001 samples: 8 segments,
63, a full wave, a full workgroup, eight workgroups); at 9 samples the two samples of a segment lie spans apart and fill the candidate
list; a mask word holds 64 directions (K = 130 on the pillars: the holds 0, 46, 72 and 129 lie in planes 0, 0, 1 and 2; K = 33 on the
wide scene: one plane)."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as F
import pose_fit_ref as PF
import pose_shortcut_ref as PS
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG = 1
FILL = -7
HANDLE = 0x1234


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def summary_of(s):
    out = {k: int(getattr(s, k)) for k, _ in L.PoseFitSummary._fields_ if k != "final"}
    out["final"] = {k: int(getattr(s.final, k)) for k, _ in L.ClearanceSummary._fields_}
    return out


def raw(g, poly, dirs, tool, holds, degree=3, spacing=8.0, max_level=6, n_samples=65, K=None, levels=True, samples=True, seg_dir=True,
        blocked=True, summary=True, spline=True, g_null=False, poly_null=False, dirs_null=False, tool_null=False, holds_null=False):
    """one raw call on prefilled outputs: dict(rc, levels, bh, th, seg_dir, blocked, s)"""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    tool = tool if isinstance(tool, L.ToolBeads) else api.torch_tool(*tool)
    holds = np.ascontiguousarray(holds, np.int32).reshape(-1)
    n_seg = max(min(int(n_samples), 1 << 16) - 1, 1)
    lv = np.full(len(holds) + 2, FILL, np.int32)
    sd, bl = np.full(n_seg + 2, FILL, np.int32), np.full(n_seg + 2, 0xA5, np.uint8)
    bh, th = C.c_void_p(HANDLE), C.c_void_p(HANDLE)
    s = L.PoseFitSummary()
    s.rounds = FILL
    s.n_blocked = FILL
    s.max_dir_turn = FILL
    p = lambda a: a.ctypes.data   # noqa: E731
    rc = g.ctx.lib.wa_grid_pose_fit_trajectory(None if g_null else g.h, None if poly_null else poly.h, degree, C.c_float(spacing), max_level,
                                               n_samples, None if dirs_null else p(dirs), len(dirs) if K is None else K,
                                               None if tool_null else C.byref(tool), None if holds_null else p(holds),
                                               p(lv) if levels else None, C.byref(bh) if spline else None, C.byref(th) if samples else None,
                                               p(sd) if seg_dir else None, p(bl) if blocked else None, C.byref(s) if summary else None)
    return dict(rc=rc, levels=lv, bh=bh, th=th, seg_dir=sd, blocked=bl, s=s)


def untouched(o):
    return ((o["levels"] == FILL).all() and (o["seg_dir"] == FILL).all() and (o["blocked"] == 0xA5).all() and o["bh"].value == HANDLE
            and o["th"].value == HANDLE and (o["s"].rounds, o["s"].n_blocked, o["s"].max_dir_turn) == (FILL, FILL, FILL))


def same(ctx, g, r, xyz, dirs, tool, holds, degree, spacing, max_level, n_samples, what):
    """one call through api.Trajectory.pose_fit against the restatement's result r: everything the call returns, bit for bit"""
    poly = api.Trajectory.from_points(ctx, xyz)
    b, samples, levels, seg_dir, blocked, s = poly.pose_fit(g, dirs, tool, holds, degree, spacing, max_level, n_samples)
    knots, cps = b.arrays()
    pts = samples.points()
    print(what, {k: v for k, v in s.items() if k != "final"}, s["final"])
    assert levels.tolist() == r["levels"].tolist(), what
    assert {k: s[k] for k in PF.SUMMARY_FIELDS} == {k: r[k] for k in PF.SUMMARY_FIELDS}, (what, s)
    assert s["final"] == r["final"], (what, s["final"], r["final"])
    assert np.array_equal(bits(knots), bits(r["knots"])) and np.array_equal(bits(cps), bits(r["cps"])), what
    assert np.array_equal(bits(pts), bits(r["samples"])), what
    assert np.array_equal(seg_dir, r["seg_dir"]) and np.array_equal(blocked, r["blocked"]), what
    out = (knots, cps, pts, levels, seg_dir, blocked, s)
    for h in (samples, b, poly):
        h.close()
    return out


# ---- the scenes of the issue, both degrees
SCENES = [("pillars4", 2001), ("box1", 1001), ("box2", 1001), ("box3", 1001), ("pillars6", 2001), ("wide", 1001)]


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", SCENES, ids=lambda c: c[0])
def test_scenes(ctx, case, degree):
    name, n = case
    s = PF.scene(name)
    g = grid_of(ctx, s["grid"])
    r = PF.fitted(name, degree, 8.0, 6, n)
    same(ctx, g, r, s["xyz"], s["dirs"], s["tool"], s["holds"], degree, 8.0, 6, n, (name, degree))
    if name in ("pillars4", "box1", "box2", "box3") and degree == 3:   # the cubic rows of the scene table
        assert r["rounds"] > 1 and r["n_blocked_first"] > 0 and r["n_blocked"] == 0 and r["n_legs_at_cap"] == 0
    if name in ("pillars6", "wide"):
        assert r["rounds"] == 1 and r["n_dir_changes"] > 0
    if name == "pillars4":
        assert sorted({int(h) >> 6 for h in s["holds"] if h >= 0}) == [0, 1, 2] and len(s["dirs"]) == 130
    if name == "wide":
        assert len(s["dirs"]) == 33
    g.close()


# ---- wave and block edges, the full candidate list, the cap path
@pytest.mark.parametrize("n", [9, 64, 65, 257])
def test_sample_counts_on_pillars4(ctx, n):
    s = PF.scene("pillars4")
    g = grid_of(ctx, s["grid"])
    for degree in (2, 3):
        r = PF.fitted("pillars4", degree, 8.0, 6, n)
        same(ctx, g, r, s["xyz"], s["dirs"], s["tool"], s["holds"], degree, 8.0, 6, n, ("pillars4", degree, n))
        if n == 9 and degree == 2:       # the cap path: not converged
            assert (r["rounds"], r["n_blocked"], r["n_legs_at_cap"]) == (8, 3, 6)
    if n == 9:   # every leg cut in four, a hold of its own for each quarter: the two spans of a segment share no control point
        t = np.array([0, .25, .5, .75], np.float32)
        x = s["xyz"]
        xyz = np.concatenate([a + (b - a) * t[:, None] for a, b in zip(x[:-1], x[1:])] + [x[-1:]]).astype(np.float32)
        held = np.arange(len(xyz) - 1, dtype=np.int32) * 3
        for degree, max_level in ((2, 0), (3, 0), (3, 6)):
            r = PF.fit(s["grid"], s["dirs"], s["tool"], xyz, held, degree, 8.0, max_level, 9, s["opened"])
            if max_level == 0:
                full = [len(PF.candidates(r["knots"], r["n_cps"], degree, r["owners"], held, i, r["dt"])) for i in range(8)]
                assert max(full) == 2 * (degree + 1), full
                assert (r["seg_dir"] >= 0).sum() >= 4 and r["n_blocked"] > 0
            same(ctx, g, r, xyz, s["dirs"], s["tool"], held, degree, 8.0, max_level, 9, ("pillars4 in quarters", degree, max_level))
    g.close()


def test_zero_length_legs(ctx):
    s = PF.scene("pillars6")
    g = grid_of(ctx, s["grid"])
    xyz = np.concatenate([s["xyz"][:1], s["xyz"][:3], s["xyz"][2:3], s["xyz"][2:], s["xyz"][-1:]])
    holds = np.concatenate([[-1], s["holds"][:2], [-1, s["holds"][2]], s["holds"][2:], [s["holds"][-1]]]).astype(np.int32)
    assert len(holds) == len(xyz) - 1 and (F.leg_lengths(xyz) == 0).sum() == 4
    for degree in (2, 3):
        r = PF.fit(s["grid"], s["dirs"], s["tool"], xyz, holds, degree, 8.0, 6, 601, s["opened"])
        same(ctx, g, r, xyz, s["dirs"], s["tool"], holds, degree, 8.0, 6, 601, ("zero legs", degree))
    g.close()


# ---- identities on the device, against wa_grid_fit_trajectory itself
def _against_fit(ctx, g, xyz, dirs, tool, holds, degree, spacing, n):
    poly = api.Trajectory.from_points(ctx, xyz)
    fb, fsamp, flev, fs = poly.fit(g, degree, spacing, 6, n)
    hit = fsamp.clearance(g)[2]
    b, samp, lev, seg_dir, blocked, s = poly.pose_fit(g, dirs, tool, holds, degree, spacing, 6, n)
    for x, y in zip(fb.arrays(), b.arrays()):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(fsamp.points()), bits(samp.points())) and np.array_equal(flev, lev)
    assert (s["rounds"], s["n_cps"], s["n_legs"], s["n_legs_at_cap"], s["max_level_used"], s["n_blocked_first"]) == \
        (fs["rounds"], fs["n_cps"], fs["n_legs"], fs["n_legs_at_cap"], fs["max_level_used"], fs["n_hit_first"])
    assert s["final"] == fs["final"] and np.array_equal(blocked, hit)
    assert (s["n_blocked"], s["first_blocked"]) == (fs["final"]["n_hit"], fs["final"]["first_hit"])
    for h in (fb, fsamp, b, samp, poly):
        h.close()
    return seg_dir, blocked, s, fs


def _identity_scenes():
    p4 = PF.scene("pillars4")
    out = [(name, (sc[0], sc[1], sc[2], sc[3]), p4["dirs"], p4["tool"], sc[4], np.arange(len(sc[4]) - 1) % 130, sp)
           for name, sc, sp in (("l_corner_long", F.l_corner(long=True), 8.0), ("diagonal_graze", F.diagonal_graze(), 1.0),
                                ("random0", F.random_scene(0), F.RANDOM_SPACING))]
    return out + [(n, PF.scene(n)["grid"], PF.scene(n)["dirs"], PF.scene(n)["tool"], PF.scene(n)["xyz"], PF.scene(n)["holds"], 8.0)
                  for n in ("pillars4", "box1")]


@pytest.mark.parametrize("degree", [2, 3])
def test_identity_a_point_tool_every_leg_held(ctx, degree):
    rounds = 0
    for name, grid, dirs, _, xyz, holds, spacing in _identity_scenes():
        g = grid_of(ctx, grid)
        held = np.where(np.asarray(holds) >= 0, holds, 0)
        seg_dir, blocked, s, fs = _against_fit(ctx, g, xyz, dirs, PS.point_tool(), held, degree, spacing, 601)
        assert s["n_no_candidate"] == 0 and ((seg_dir >= 0) == (blocked == 0)).all(), name
        rounds = max(rounds, fs["rounds"])
        g.close()
    assert rounds > 1


@pytest.mark.parametrize("degree", [2, 3])
def test_identity_b_no_leg_held(ctx, degree):
    for name, grid, dirs, tool, xyz, holds, spacing in _identity_scenes():
        g = grid_of(ctx, grid)
        seg_dir, _, s, _ = _against_fit(ctx, g, xyz, dirs, tool, np.full(len(xyz) - 1, -1), degree, spacing, 601)
        assert s["n_no_candidate"] == 600 and (seg_dir == -1).all() and (s["n_dir_changes"], s["max_dir_turn"]) == (0, 0), name
        g.close()


# ---- NULL optional outputs, repeatability, errors
def test_null_optional_outputs_and_repeatability(ctx):
    s = PF.scene("pillars4")
    g = grid_of(ctx, s["grid"])
    poly = api.Trajectory.from_points(ctx, s["xyz"])
    r = PF.fitted("pillars4", 3, 8.0, 6, 257)
    full = raw(g, poly, s["dirs"], s["tool"], s["holds"], n_samples=257)
    again = raw(g, poly, s["dirs"], s["tool"], s["holds"], n_samples=257)
    bare = raw(g, poly, s["dirs"], s["tool"], s["holds"], n_samples=257, levels=False, samples=False, seg_dir=False, blocked=False)
    want = {k: r[k] for k in PF.SUMMARY_FIELDS}
    for o in (full, again, bare):
        assert o["rc"] == 0, ctx.lib.wa_last_error(ctx.h)
        got = summary_of(o["s"])
        assert {k: got[k] for k in PF.SUMMARY_FIELDS} == want and got["final"] == r["final"]
    for o in (full, again):
        assert np.array_equal(o["seg_dir"][:256], r["seg_dir"]) and (o["seg_dir"][256:] == FILL).all()
        assert np.array_equal(o["blocked"][:256], r["blocked"]) and (o["blocked"][256:] == 0xA5).all()
        assert np.array_equal(o["levels"][:-2], r["levels"]) and (o["levels"][-2:] == FILL).all()
    assert (bare["levels"] == FILL).all() and (bare["seg_dir"] == FILL).all() and (bare["blocked"] == 0xA5).all() and bare["th"].value == HANDLE
    splines = [api.Bspline.adopt(ctx, o["bh"], 3, 3, r["n_cps"] - 6) for o in (full, again, bare)]
    for b in splines:
        knots, cps = b.arrays()
        assert np.array_equal(bits(knots), bits(r["knots"])) and np.array_equal(bits(cps), bits(r["cps"]))
    pts = [api.Trajectory(ctx, o["th"]) for o in (full, again)]
    assert np.array_equal(bits(pts[0].points()), bits(r["samples"])) and np.array_equal(bits(pts[1].points()), bits(r["samples"]))
    for h in splines + pts + [poly]:
        h.close()
    g.close()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    s = PF.scene("wide")
    g = grid_of(ctx, s["grid"])
    poly = api.Trajectory.from_points(ctx, s["xyz"])
    K = len(s["dirs"])
    a = (g, poly, s["dirs"], s["tool"], s["holds"])
    other = api.Context(0)
    foreign = api.Trajectory.from_points(other, s["xyz"])
    one = api.Trajectory.from_points(ctx, s["xyz"][:1])
    bad_xyz = s["xyz"].copy()
    bad_xyz[2, 1] = np.inf
    infinite = api.Trajectory.from_points(ctx, bad_xyz)
    zero_dir = s["dirs"].copy()
    zero_dir[3] = 0
    nan_dir = s["dirs"].copy()
    nan_dir[0, 2] = np.nan
    no_beads, far_bead, big_bead = api.torch_tool(*s["tool"]), api.torch_tool(*s["tool"]), api.torch_tool(*s["tool"])
    no_beads.n_beads = 0
    far_bead.dist16[0] = 65537
    big_bead.r2[0] = -1
    low, high = s["holds"].copy(), s["holds"].copy()
    low[1], high[-1] = -2, K
    cases = {
        "NULL grid": raw(*a, g_null=True), "NULL polyline": raw(*a, poly_null=True), "NULL summary": raw(*a, summary=False),
        "NULL spline output": raw(*a, spline=False), "another context": raw(g, foreign, *a[2:]), "one point": raw(g, one, s["dirs"], s["tool"], []),
        "degree 1": raw(*a, degree=1), "degree 4": raw(*a, degree=4), "spacing 0": raw(*a, spacing=0.0), "spacing < 0": raw(*a, spacing=-1.0),
        "spacing nan": raw(*a, spacing=float("nan")), "spacing inf": raw(*a, spacing=float("inf")), "max_level -1": raw(*a, max_level=-1),
        "max_level 9": raw(*a, max_level=9), "1 sample": raw(*a, n_samples=1), "2^33 + 1 samples": raw(*a, n_samples=(1 << 33) + 1),
        "infinite coordinate": raw(g, infinite, *a[2:]), "too many control points": raw(*a, spacing=1e-7),
        "NULL dirs": raw(*a, dirs_null=True), "K 0": raw(*a, K=0), "K 257": raw(*a, K=257), "NULL tool": raw(*a, tool_null=True),
        "zero direction": raw(g, poly, zero_dir, s["tool"], s["holds"]), "nan direction": raw(g, poly, nan_dir, s["tool"], s["holds"]),
        "no beads": raw(g, poly, s["dirs"], no_beads, s["holds"]), "bead too far": raw(g, poly, s["dirs"], far_bead, s["holds"]),
        "negative r2": raw(g, poly, s["dirs"], big_bead, s["holds"]), "NULL leg_hold": raw(*a, holds_null=True),
        "hold -2": raw(g, poly, s["dirs"], s["tool"], low), "hold K": raw(g, poly, s["dirs"], s["tool"], high),
    }
    for what, o in cases.items():
        assert o["rc"] == ARG, (what, o["rc"])
        assert untouched(o), what
    ok = raw(*a, n_samples=65)
    assert ok["rc"] == 0 and not untouched(ok)
    api.Bspline.adopt(ctx, ok["bh"], 3, 3, int(ok["s"].n_cps) - 6).close()
    api.Trajectory(ctx, ok["th"]).close()
    for h in (foreign, one, infinite, poly):
        h.close()
    other.close()
    g.close()
