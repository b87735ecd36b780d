"""Named scenes that take the timing calls (include/weldacs.h: wa_traj_retime, wa_traj_retime_stops, wa_traj_retime_jerk, wa_traj_tick_axes,
wa_traj_tick_axes_stops) away from small magnitudes: prefix sums of U that wrap modulo 2^64, caps saturated at 2^61, sums of A, D, L and
durations just under 2^61, keys C * 4 + kind at 2^63, int64 -> double conversions above 2^53, caps of 0 and 1 quantum inside a path.
Every other scene of the suite is 1 - 5 units long at speeds of about 1.  No GPU, no product code.

A scene is (xyz, lim, tick, W, dwell, v_limit, seg_tag).  Each carries an assertion on the RESTATEMENT's result (jerk_ref.retime_jerk)
that it sits in the regime it is named for: reference(name) evaluates it, so a scene that drifts out of its regime fails wherever it is
used.  reference(name) is computed once per process and must be left unchanged by its users.

The pairs at the end stand one step apart on both sides of a refusal; their values are found with the restatement, none by hand."""
import functools

import numpy as np

import jerk_ref as J
import retime_ref as R
import stops_ref as S

Q = R.Q
CAP = R.CAP_INF


def total(a):
    """the exact sum of an array of int64 >= 0 as a Python integer: the high and the low 32 bits summed apart (fewer than 2^31 entries,
    so neither sum passes 2^63)"""
    a = np.asarray(a, np.int64)
    assert len(a) < (1 << 31) and (a >= 0).all()
    return (int((a >> 32).sum()) << 32) + int((a & 0xffffffff).sum())


# ------------------------------------------------------------------ the scenes
def _wrap(W):
    return R.line(9, float(2 ** 25)), R.limits(v_max=1e5, acc=1.0, dec=1.0), 1.0, W, None, None, None


def _wrap_regime(r):
    assert r["summary"]["length_q"] == 2 ** 55
    assert total(r["U"]) > 2 ** 66                                   # the prefix sums wrap several times
    W = r["jerk"]["window"]
    assert W * 2 ** 55 < 2 ** 62 <= 128 * 2 ** 55 and W <= 127       # 127 is the last window rule 48 accepts


def _past_double():
    return R.line(17, 4096.0), R.limits(v_max=50.0, acc=20.0, dec=10.0), 0.02, 8, None, None, None


def _past_double_regime(r):
    assert 2 ** 53 < total(r["U"]) < 2 ** 64                         # no wrap, but past what a double holds


def _stops(W):
    """test_gpu_jerk.stops_scene with its coordinates scaled by 2^20 (exact in fp32): three pieces joined by stops"""
    a = R.densify([[0, 0, 0], [0.93, 0, 0]], 60)
    b = R.densify([[0.93, 0, 0], [0.93, 1.1, 0]], 50)
    c = R.densify([[0.93, 1.1, 0], [2, 1.1, 0.5]], 40)
    xyz, dwell, _ = S.with_stops([a, b, c], [40.0, 16.0])
    xyz = (xyz * np.float32(2 ** 20)).astype(np.float32)
    v_limit = np.full(len(xyz), 5000.0, np.float32)
    v_limit[75:95] = 300.0
    tag = (np.arange(len(xyz) - 1) % 251 + 1).astype(np.uint8)
    return xyz, R.limits(v_max=4000.0, acc=200.0, dec=200.0, a_lat=1e4), 0.5, W, dwell, v_limit, tag


def _stops_regime(r):
    j = r["jerk"]
    assert total(r["U"]) > 2 ** 61
    assert j["n_rest_ticks"] > 0 and j["n_short_rests"] == 0 and r["stops"]["n_stops"] == 2
    assert J.rest_ticks_per_stop(r).tolist() == [80, 32]             # 40 s and 16 s at a tick of 0.5 s
    assert j["n_lowered"] > 0 or j["window"] == 1


def _helix():
    xyz = (R.helix(4097, radius=0.5, pitch=0.05, turns=1.5).astype(np.float64) * 2 ** 16).astype(np.float32)
    v_limit = np.full(len(xyz), 5000.0, np.float32)
    v_limit[1500:1520] = 400.0
    return xyz, R.limits(v_max=3000.0, acc=500.0, dec=800.0, a_lat=30.0), 0.25, 33, None, v_limit, None


def _helix_regime(r):
    n = r["summary"]["n"]
    assert n == 4097 and 2 ** 48 < r["GL"][-1] < 2 ** 49
    on2 = ((r["bound"] & 1) != 0) & (((r["bound"] >> 4) & 3) == R.KIND_CURV)
    assert 2 * int(on2.sum()) > n and 2 * r["summary"]["n_bound"][2] > n   # kind 2 binds on most samples
    assert r["jerk"]["n_lowered"] > 0


def _saturated(n, acc, dec):
    return R.line(n, 1024.0), R.limits(v_max=1e9, acc=acc, dec=dec), 2.0 ** -12, 3, None, None, None


def _saturated_regime(r):
    assert (r["C13"] == CAP).all() and (r["C"][1:-1] == CAP).all()   # every interior cap is saturated
    big = 2.0 ** 60.9
    a, d = total(r["A"]), total(r["D"])
    assert (a >= big or d >= big) and max(a, d) < CAP
    on_cap = (r["bound"] & 1) != 0
    assert not on_cap[1:-1].any() and ((r["bound"][1:-1] & 6) != 0).all()   # only ramps bind
    if r["jerk"]["window"] > 1:
        assert r["jerk"]["reach_q"] > 0                              # the keys of rule 49 are 2^61 * 4 + 1 >= 2^63


def _long():
    return R.line(2049, 2.0 ** 30 * 0.999), R.limits(v_max=1e4, acc=0.999, dec=0.5), 16.0, 4, None, None, None


def _long_regime(r):
    assert r["summary"]["length_q"] > 2.0 ** 59.9 and 2.0 ** 60.9 < total(r["A"]) < CAP
    assert r["jerk"]["window"] * r["summary"]["length_q"] < 2 ** 62


def _slow():
    return R.line(33, float(2 ** 15)), R.limits(v_max=2.0 ** -15 * 1.01, acc=1.0, dec=1.0), float(2 ** 20), 5, None, None, None


def _slow_regime(r):
    assert (r["C13"] == 1).all() and (r["C"][1:-1] == 1).all()       # every interior cap is one quantum
    assert 2 ** 60 < r["summary"]["time_q"] < CAP


def _tiny(W):
    v_limit = np.full(41, 5.0, np.float32)
    v_limit[10] = 1e-5
    v_limit[20] = 4e-5
    v_limit[30:33] = 3.1e-5
    return R.line(41, 1.0 / 64), R.limits(v_max=1.0, acc=1.0, dec=1.0), 0.25, W, None, v_limit, None


def _tiny_regime(r):
    s = r["summary"]
    if r["jerk"]["window"] == 1:
        assert r["w_q"][10] == 0 and r["w_q"][20] == 1 and (r["w_q"][30:33] == 1).all() and r["stops"]["n_stops"] == 0
        assert r["C"][10] == 0 and r["C"][20] == 1
    else:
        assert (r["Cl"] == 0).all() and r["jerk"]["n_lowered"] == s["n"] - 1   # (sample 10's own cap is 0 already)
        assert s["n_triangle"] == s["n"] - 1 and s["peak_w_q"] == 0


def _third_level():
    """the third scan level together with the wrap: the duration comes from the restatement"""
    xyz, lim = R.line(9, float(2 ** 14)), R.limits(v_max=1e4, acc=2.0, dec=2.0)
    duration = R.retime(xyz, lim, None, None, 1.0, False)["summary"]["time_q"] / R.QF
    return xyz, lim, 0.98 * duration / (1 << 22), 64, None, None, None


def _third_level_regime(r):
    assert r["jerk"]["n_in"] > (1 << 22) + 1 and total(r["U"]) > 2 ** 64
    assert r["summary"]["n_on_cap"] == 2                             # v_max does not bind: only the end points are on their caps


ACC_LAST = 2.0 ** 20 * 0.999   # scene 5's ramps: the sum of A (of D) is 2^61 * 0.999; at 2^20 it is 2^61 and the call is refused
SCENES = {
    "wrap_w1": (lambda: _wrap(1), _wrap_regime), "wrap_w2": (lambda: _wrap(2), _wrap_regime), "wrap_w8": (lambda: _wrap(8), _wrap_regime),
    "wrap_w127": (lambda: _wrap(127), _wrap_regime),
    "past_double": (_past_double, _past_double_regime),
    "stops_w1": (lambda: _stops(1), _stops_regime), "stops_w4": (lambda: _stops(4), _stops_regime),
    "stops_w25": (lambda: _stops(25), _stops_regime),
    "helix": (_helix, _helix_regime),
    "saturated_acc": (lambda: _saturated(33, ACC_LAST, 2.0 ** 19), _saturated_regime),
    "saturated_dec": (lambda: _saturated(33, 2.0 ** 18, ACC_LAST), _saturated_regime),
    "saturated_2049": (lambda: _saturated(2049, ACC_LAST, ACC_LAST), _saturated_regime),
    "long": (_long, _long_regime),
    "slow": (_slow, _slow_regime),
    "tiny_w1": (lambda: _tiny(1), _tiny_regime), "tiny_w5": (lambda: _tiny(5), _tiny_regime),
    "third_level": (_third_level, _third_level_regime),
}
SMALL = [k for k in SCENES if k != "third_level"]                    # <= 4 097 samples, and all but the helix <= ~12 000 ticks
PROFILE_SCENES = ["stops_w4", "helix", "saturated_acc", "saturated_dec", "saturated_2049", "long", "slow", "tiny_w1"]   # scenes 3 - 8
AXES_SCENES = ["stops_w4", "saturated_acc", "saturated_2049", "long", "slow"]                                        # scenes 3, 5, 6, 7


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """jerk_ref.retime_jerk on the scene, its regime asserted; retime_ref.retime's A, D, F and ds ride along"""
    xyz, lim, tick, W, dwell, v_limit, seg_tag = scene(name)
    r = J.retime_jerk(xyz, lim, dwell, W, v_limit, None, tick, seg_tag)
    base = R.retime(xyz, lim, v_limit, None, tick, False)
    r = dict(r, A=base["A"], D=base["D"], ds=base["ds"])
    assert r["ticks"] is not None and r["s_q"] is not None, name
    SCENES[name][1](r)
    return r


@functools.lru_cache(maxsize=None)
def profile_reference(name, stops):
    """retime_ref.retime (stops False: the dwells are ignored) or stops_ref.retime_stops on the scene, with its ticks"""
    xyz, lim, tick, W, dwell, v_limit, seg_tag = scene(name)
    reference(name)                                                  # (the regime)
    return S.retime_stops(xyz, lim, dwell, v_limit, None, tick) if stops else R.retime(xyz, lim, v_limit, None, tick)


# ------------------------------------------------------------------ pairs one step apart on both sides of a refusal
def accepted(call):
    try:
        call()
        return True
    except ValueError:
        return False


def last_accepted_double(ok, lo, hi):
    """(the largest double x in [lo, hi) with ok(x), the next double above it); ok(lo) and not ok(hi), ok monotone.  Bisection over
    the bit patterns of positive doubles, which are ordered like the doubles."""
    assert 0 < lo < hi and ok(lo) and not ok(hi)
    a, b = (int(np.float64(x).view(np.int64)) for x in (lo, hi))
    while b - a > 1:
        m = (a + b) // 2
        if ok(float(np.int64(m).view(np.float64))):
            a = m
        else:
            b = m
    return float(np.int64(a).view(np.float64)), float(np.int64(b).view(np.float64))


PAIR_TICK = float(2 ** 24)   # 2^54 quanta: a dwell of nearly 2^61 quanta is 128 ticks, the window's extension 4 of them
PAIR_W = 5


def dwell_only_scene():
    """two samples at one place and the stop between them: the duration IS the extended dwell dq + (W - 1) * tick_q"""
    xyz = np.zeros((2, 3), np.float32)
    xyz[:, 0] = 3.0
    return xyz, R.limits(v_max=1.0, acc=1.0, dec=1.0)


def moving_scene():
    """a line of 21 samples with a stop in the middle: the duration is the dwell plus the time of the motion"""
    a = R.line(11, 1.0)
    b = a + np.array([1.0, 0, 0], np.float32)
    xyz, dwell, at = S.with_stops([a, b], [1.0])
    return xyz, R.limits(v_max=1.0, acc=1.0, dec=1.0), at[0]


@functools.lru_cache(maxsize=None)
def extended_dwell_pair():
    """(xyz, lim, dwell of the last accepted call, dwell of the first refused one) for retime_jerk at PAIR_W, PAIR_TICK"""
    xyz, lim = dwell_only_scene()
    ok = lambda d: accepted(lambda: J.retime_jerk(xyz, lim, np.array([d]), PAIR_W, tick=PAIR_TICK, want_ticks=False))
    good, bad = last_accepted_double(ok, 1.0, 2.0 ** 31)
    r = J.retime_jerk(xyz, lim, np.array([good]), PAIR_W, tick=PAIR_TICK)
    ext = (PAIR_W - 1) * r["tick_q"]
    assert CAP - 2 ** 9 <= int(r["dq"][0]) + ext < CAP and r["summary"]["time_q"] == int(r["dq"][0]) + ext   # (a double near 2^31 has steps of 2^8 quanta)
    assert int(np.rint(bad * R.QF)) + ext >= CAP > int(np.rint(bad * R.QF))   # the dwell alone would pass rule 40
    return xyz, lim, np.array([good]), np.array([bad])


@functools.lru_cache(maxsize=None)
def duration_pair(W):
    """(xyz, lim, dwell of the last accepted call, of the first refused one) where only the DURATION reaches 2^61: W = 1 for
    retime_stops (and retime_jerk with a window of one tick), PAIR_W for retime_jerk"""
    xyz, lim, at = moving_scene()
    base = np.full(len(xyz) - 1, -1.0)

    def with_dwell(d):
        out = base.copy()
        out[at] = d
        return out
    call = lambda d, ticks=False: J.retime_jerk(xyz, lim, with_dwell(d), W, tick=PAIR_TICK, want_ticks=ticks)
    good, bad = last_accepted_double(lambda d: accepted(lambda: call(d)), 1.0, 2.0 ** 31)
    r = call(good, True)
    ext = (W - 1) * r["tick_q"]
    assert CAP - 2 ** 9 <= r["summary"]["time_q"] < CAP
    assert int(np.rint(bad * R.QF)) + ext < CAP                      # the first refused dwell passes rules 40 and 48: the duration refuses it
    if W == 1:
        assert accepted(lambda: S.retime_stops(xyz, lim, with_dwell(good), tick=PAIR_TICK))
        assert not accepted(lambda: S.retime_stops(xyz, lim, with_dwell(bad), tick=PAIR_TICK))
    return xyz, lim, with_dwell(good), with_dwell(bad)
