"""The definition of the jerk-limited controller ticks (include/weldacs.h rules 48 - 55, restated in tests/jerk_ref.py) held against
what it claims, without a device: the jerk bound, the speed at the place against the caps there, the negative control without the
lowering, full rests, end values, the window of one tick, odd shapes, the per-tick scalar form and the refusals.

Scenes: right_angle(200), slab_scene(150) (v_max 2, acc = dec 4, v_near 0.3, near_d2 9), random_scene(0 .. 5) and three pieces joined by
stops of 0.5 and 0.2 s with a dip in v_limit.  Windows from {1, 2, 5, 7, 8, 16, 25, 33}."""
import numpy as np
import pytest

import jerk_ref as J
import retime_ref as R
import stops_ref as S

LIM = R.limits(v_max=1.0, acc=2.0, dec=2.0, a_lat=0.5)
SLAB_LIM = R.limits(v_max=2, acc=4, dec=4, v_near=0.3, near_d2=9)
WINDOWS = (1, 2, 5, 7, 8, 16, 25, 33)


def stops_scene():
    a = R.densify([[0, 0, 0], [0.93, 0, 0]], 60)
    b = R.densify([[0.93, 0, 0], [0.93, 1.1, 0]], 50)
    c = R.densify([[0.93, 1.1, 0], [2, 1.1, 0.5]], 40)
    xyz, dwell, at = S.with_stops([a, b, c], [0.5, 0.2])
    v_limit = np.full(len(xyz), 5.0, np.float32)
    v_limit[75:95] = 0.3
    return xyz, dwell, v_limit, at


def scenes():
    """(name, xyz, lim, dwell, v_limit, grid, tick)"""
    yield "right_angle", R.right_angle(200), LIM, None, None, None, 0.004
    grid, xyz = R.slab_scene(150)
    yield "slab", xyz, SLAB_LIM, None, None, grid, 0.004
    for seed in range(6):
        grid, xyz, lim, v_limit, tick = R.random_scene(seed)
        yield "random%d" % seed, xyz, lim, None, v_limit, grid, tick
    xyz, dwell, v_limit, _ = stops_scene()
    yield "with_stops", xyz, LIM, dwell, v_limit, None, 0.004


SCENES = list(scenes())


@pytest.fixture(scope="module")
def results():
    """every scene at every window, computed once"""
    return {(s[0], W): J.retime_jerk(s[1], s[2], s[3], W, s[4], s[5], s[6]) for s in SCENES for W in WINDOWS}


def test_the_jerk_bound(results):
    """Delta^3 of the window sums is a difference of two Delta^2 U; the floors add less than 4"""
    for (name, W), r in results.items():
        j = r["jerk"]
        assert j["max_d3"] * W <= 2 * j["in_max_d2"] + 4 * W, (name, W, j)
        assert j["window"] == W and j["n_ticks"] == j["n_in"] + W - 1 == len(r["s_q"])


def test_speed_at_the_place_keeps_the_caps_there(results):
    """a filtered step is within 2 quanta (the rint in U, the floor in S) of what the largest cap between its ends allows"""
    worst = 0.0
    for (name, W), r in results.items():
        tick = [s for s in SCENES if s[0] == name][0][6]
        e = J.speed_excess(r, tick)
        worst = max(worst, e)
        assert e <= 2.0, (name, W, e)
    print("largest excess: %.3f quanta" % worst)


@pytest.mark.parametrize("W", [5, 16])
def test_without_the_lowering_the_slab_scene_breaks_its_cap(W):
    grid, xyz = R.slab_scene(150)
    r = J.retime_jerk(xyz, SLAB_LIM, None, W, None, grid, 0.004, lower=False)
    e = J.speed_excess(r, 0.004)
    print("W = %d, no lowering: %.0f quanta over the cap" % (W, e))
    assert e > 1e4 and r["jerk"]["reach_q"] == 0 and r["jerk"]["n_lowered"] == 0
    assert J.speed_excess(J.retime_jerk(xyz, SLAB_LIM, None, W, None, grid, 0.004), 0.004) <= 2.0


def test_rests_are_full_and_ends_are_exact(results):
    for (name, W), r in results.items():
        j = r["jerk"]
        assert j["n_short_rests"] == 0 and j["n_back"] == 0, (name, W, j)
        assert r["s_q"][0] == 0 and r["s_q"][-1] == r["summary"]["length_q"], (name, W)
        assert np.array_equal(r["ticks"][0], np.asarray(SCENES[[s[0] for s in SCENES].index(name)][1], np.float32)[0])
    xyz, dwell, v_limit, at = stops_scene()
    for W in (1, 4, 25):
        r = J.retime_jerk(xyz, LIM, dwell, W, v_limit, None, 0.004)
        assert J.rest_ticks_per_stop(r).tolist() == [125, 50], (W, J.rest_ticks_per_stop(r))
        assert r["stops"] == dict(n_stops=2, n_stop_samples=4, dwell_q=int(0.5 * J.Q) + int(np.rint(0.2 * J.QF)))


def test_a_window_of_one_tick_is_retime_stops():
    differ = total = 0
    for name, xyz, lim, dwell, v_limit, grid, tick in SCENES:
        r = J.retime_jerk(xyz, lim, dwell, 1, v_limit, grid, tick)
        s = S.retime_stops(xyz, lim, dwell, v_limit, grid, tick)
        for k in ("time_q", "w_q", "bound"):
            assert r[k].dtype == s[k].dtype and r[k].tobytes() == s[k].tobytes(), (name, k)
        assert r["summary"] == s["summary"] and r["stops"] == s["stops"], name
        assert np.array_equal(r["s_q"], r["U"]) and r["jerk"]["reach_q"] == 0
        # half a quantum of lambda and one fp32 rounding
        a, b = r["ticks"].astype(np.float64), s["ticks"].astype(np.float64)
        allow = 2.0 ** -30 + np.spacing(np.abs(s["ticks"])).astype(np.float64)
        assert (np.abs(a - b) <= allow).all(), (name, float((np.abs(a - b) - allow).max()))
        differ += int((a != b).sum())
        total += a.size
    print("%d of %d coordinates differ at all" % (differ, total))


def test_odd_shapes():
    xyz = R.right_angle(20, 0.2)
    for W in (500, 5000):   # more ticks in the window than the profile has (no curvature cap: the corner is taken at v_max)
        r = J.retime_jerk(xyz, R.limits(v_max=1.0, acc=2.0, dec=2.0), None, W, tick=0.004)
        j = r["jerk"]
        assert W > j["n_in"] and j["n_ticks"] == j["n_in"] + W - 1 and j["n_back"] == 0
        assert r["s_q"][0] == 0 and r["s_q"][-1] == r["summary"]["length_q"]
        assert j["max_d3"] * W <= 2 * j["in_max_d2"] + 4 * W
    # 300 repeated samples without a stop: no rest tick, the ticks there are p_i of the run's last segment
    a = R.densify([[0, 0, 0], [1.0, 0, 0]], 40)
    b = R.densify([[1.0, 0, 0], [1.0, 0.6, 0.2]], 30)
    xyz = np.concatenate([a, np.repeat(a[-1:], 300, 0), b[1:]]).astype(np.float32)
    r = J.retime_jerk(xyz, LIM, None, 7, tick=0.004)
    assert r["jerk"]["n_rest_ticks"] == 0 and r["jerk"]["n_back"] == 0
    in_run = (r["seg"] >= 40) & (r["seg"] < 340)   # (the run's segments have no length: only a tick exactly at its place lies on one)
    assert (r["s_q"][in_run] == r["GL"][40]).all() and (r["seg"][in_run] == 339).all() and (r["ticks"][in_run] == a[-1]).all()
    assert (r["seg"] < 40).any() and (r["seg"] >= 340).any()
    # stops on segment 0 and on segment n - 2, three stops in a row with a 0-second dwell among them
    p = R.densify([[0, 0, 0], [0.5, 0, 0]], 25)
    q = R.densify([[0.5, 0, 0], [0.5, 0.4, 0]], 20)
    xyz, dwell, at = S.with_stops([p[:1], p, q, q[-1:]], [0.05, [0.1, 0.0, 0.07], 0.03])
    assert at[0] == 0 and at[-1] == len(xyz) - 2
    tag = (np.arange(len(xyz) - 1) + 1).astype(np.uint8)
    tq = int(np.rint(0.004 * J.QF))
    for W in (1, 2, 6):
        r = J.retime_jerk(xyz, LIM, dwell, W, tick=0.004, seg_tag=tag)
        got = J.rest_ticks_per_stop(r)
        assert r["jerk"]["n_short_rests"] == 0 and r["jerk"]["n_back"] == 0
        assert got[2] == got[3] == 0 and got[1] >= int(np.rint((0.1 + 0.07) * J.QF)) // tq   # (the row acts as one stop, the first one's)
        assert got[0] >= int(np.rint(0.05 * J.QF)) // tq and got[4] >= int(np.rint(0.03 * J.QF)) // tq
        assert (r["tag"][r["rest"] & (r["seg"] == at[1])] == tag[at[1]]).all()


def test_the_scalar_form_gives_the_same_ticks():
    xyz, dwell, v_limit, _ = stops_scene()
    small = [(R.right_angle(12, 0.1), LIM, None, None, None, 0.01, 5), (xyz[40:80], LIM, dwell[40:79], v_limit[40:80], None, 0.01, 3)]
    grid, gx, lim, vl, tick = R.random_scene(4)
    small.append((gx[:60], lim, None, vl[:60] if vl is not None else None, grid, 0.05, 4))
    for pts, lim, dw, vl, grid, tick, W in small:
        tag = (np.arange(len(pts) - 1) % 5).astype(np.uint8)
        r = J.retime_jerk(pts, lim, dw, W, vl, grid, tick, tag)
        s_q, segs, rests, pos, tags = J.retime_jerk_scalar(pts, lim, dw, W, vl, grid, tick, tag)
        assert s_q == r["s_q"].tolist() and segs == r["seg"].tolist() and rests == r["rest"].tolist() and tags == r["tag"].tolist()
        assert pos.tobytes() == r["ticks"].tobytes()


def test_every_refusal_of_rule_48():
    xyz, dwell, v_limit, _ = stops_scene()
    ok = lambda **kw: J.retime_jerk(**dict(dict(xyz=xyz, lim=LIM, dwell=dwell, window=4, v_limit=v_limit, tick=0.004), **kw))
    ok()
    bad = [dict(window=0), dict(window=(1 << 20) + 1), dict(window=2.5),
           dict(lim=R.limits(v_max=1e9, acc=2, dec=2), tick=1e4, window=1 << 20),            # R_q
           dict(tick=2.0 ** 30, window=1 << 20, dwell=None),                                   # (W - 1) * tick_q
           dict(dwell=np.where(dwell >= 0, 2.0 ** 31 - 1.0, -1.0), window=1 << 10, tick=2.0 ** 21),   # dq + (W - 1) * tick_q
           dict(want_tags=True),                                                               # tag_out without seg_tag
           dict(tick=float("nan")), dict(lim=R.limits(v_max=0, acc=2, dec=2)), dict(dwell=np.full(len(xyz) - 1, 0.1))]   # rules 7 and 40
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    far, fl = R.line(3, 8192.0), R.limits(v_max=100.0, acc=100.0, dec=100.0)   # W * length_q: 2^20 * 2^43
    J.retime_jerk(far, fl, None, 1 << 18, tick=1.0, want_ticks=False)
    with pytest.raises(ValueError):
        J.retime_jerk(far, fl, None, 1 << 20, tick=1.0, want_ticks=False)
    for args in ((0.0, 1, 1, 1), (1, 1, float("inf"), 1), (1, 1, 1, -1.0), (1e9, 1, 1e-9, 1e-9)):
        with pytest.raises(ValueError):
            J.jerk_window(*args)
    assert J.jerk_window(2.0, 4.0, 1000.0, 0.001) == 8 and J.jerk_window(1.0, 1.0, 1e9, 1.0) == 1
