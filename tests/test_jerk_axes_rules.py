"""CPU checks of the restatement of the torch axes at jerk-limited ticks (tests/jerk_axes_ref.py, rules 56 - 60 of include/weldacs.h):
its array form against a plain per-tick loop, and the properties the rules are there for.  No GPU, no product code.

The step of a turn in place.  Over the R rest ticks of a stop the axis is v(lambda) = q_a + (q_e - q_a) * lambda at lambda = j / R,
normalised and rounded by rule 1.  Consecutive v differ by exactly (q_e - q_a) / R.  Normalising two vectors x, y changes their distance
by at most 1 / sqrt(|x| |y|) (from |x - y|^2 >= |x| |y| * |x/|x| - y/|y||^2), and the chord between the two quantised axes passes inside
the sphere, so |v| <= 16384 and that factor is at least 1 / 16384: it is 1 for a small turn and grows towards the middle of a wide
one (rule 42 says the same of a dwell).  Rule 1 rounds every component to the nearest integer: each axis moves by at most
sqrt(3) / 2 units of 2^-14, a step by at most sqrt(3).  So, in units of 2^-14,
    chord(qt_j, qt_j+1) <= 16384 * |q_e - q_a| / (R * sqrt(|v_j| |v_j+1|)) + sqrt(3) + 1e-6
(the 1e-6 covers the few float64 roundings of v, its length and the division, each below 2^-50 relative).  The tick in front of the
rest (axis q_a) and the one behind it (axis q_e) are the chain's ends at lambda = 0 and 1."""
import numpy as np
import pytest

import jerk_axes_ref as X
import jerk_ref as J
import retime_ref as R

K, T = X.K, X.T
LIM = R.limits(v_max=4.0, acc=8.0, dec=8.0)


def stop_scene(q_a, q_e, dwell, before=1.0, after=1.0, joint=None):
    a = R.densify([[2, 12, 8], [2 + before, 12, 8]], 6)
    b = R.densify([[2 + before, 12, 8], [2 + before + after, 12, 8]], 5)
    joint = [dwell] if joint is None else joint
    xyz, dw = X.polyline([(a, []), (b, joint)])
    q = np.empty((len(xyz), 3), np.int64)
    q[:len(a)] = q_a
    q[len(a):] = q_e
    return xyz, q, dw, len(a) - 1


@pytest.mark.parametrize("seed", range(40))
def test_the_array_form_is_the_per_tick_loop(seed):
    c = X.random_case(seed)
    W = (1, 2, 3, 7, 20)[seed % 5]
    r = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c["dwell"], W, None, c["grid"], c["tool"], c["near_add"], c["tick"], c["tag"])
    loop = X.retime_jerk_axes_scalar(c["xyz"], c["q"], c["lim"], c["dwell"], W, None, c["grid"], c["tick"])
    assert r["qt"].tolist() == loop
    assert np.array_equal(r["axes"], (r["qt"].astype(np.float64) / 16384.0).astype(np.float32)) and set(np.unique(r["blocked"])) <= {0, 1}


def test_the_random_cases_cover_what_they_are_for():
    seen = dict(rest=0, turning=0, blocked=0, near=0, run=0, no_dwell=0, zero_len=0)
    for seed in range(40):
        c = X.random_case(seed)
        r = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c["dwell"], 3, None, c["grid"], c["tool"], c["near_add"], c["tick"])
        s = r["axes_summary"]
        assert 2 <= len(c["xyz"]) <= 40 and s["n_ticks"] < 8000
        seen["rest"] += s["n_rest_ticks"] > 0
        seen["turning"] += s["n_turning_rests"] > 0
        seen["blocked"] += 0 < s["n_blocked"] < s["n_ticks"]
        seen["near"] += s["n_near"] > 0
        seen["no_dwell"] += c["dwell"] is None
        seen["zero_len"] += bool(((r["L"] == 0) & (r["dq"] < 0)).any())
        f = np.flatnonzero(r["dq"] >= 0)
        a, e = X.runs(r["GL"], f)
        seen["run"] += bool(((a < f) | (e > f + 1)).any())
    assert all(v >= 3 for v in seen.values()), seen


def test_equal_axes_give_that_axis_at_every_tick():
    q1 = X.fixed_axis((0.3, -0.5, 0.8))
    assert np.array_equal(K.quantise_rows(q1[None].astype(np.float64))[0], q1)   # (rule 1 maps it to itself; not every quantised axis is)
    for seed in (0, 2, 4, 8):
        c = X.random_case(seed)
        q = np.tile(q1, (len(c["xyz"]), 1))
        for W in (1, 5, 40):
            r = X.retime_jerk_axes(c["xyz"], q, c["lim"], c["dwell"], W, None, c["grid"], c["tool"], c["near_add"], c["tick"])
            s = r["axes_summary"]
            assert (r["qt"] == q1).all() and s["max_tick_turn"] == 0 and s["max_rest_turn"] == 0 and s["n_turning_rests"] == 0
            assert s["min_turn_ticks"] == 0 and s["n_rest_ticks"] == r["jerk"]["n_rest_ticks"]


def test_a_rest_between_equal_axes_is_constant():
    """q_a = q_e with other axes on the samples inside the run: the rest ticks all carry q_a"""
    q_a = X.fixed_axis((0.2, 0.9, -0.1))
    xyz, q, dw, f = stop_scene(q_a, q_a, None, joint=[-1.0, 0.08, -1.0])
    q[f + 1], q[f + 2] = T.quantise_all([[1, 0, 0], [0, 0, -1]])   # (inside the run: passed over)
    for W in (1, 4):
        r = X.retime_jerk_axes(xyz, q, LIM, dw, W, tick=0.01)
        k = np.flatnonzero(r["rest"])
        assert len(k) >= 8 and (r["qt"][k] == q_a).all() and r["axes_summary"]["n_turning_rests"] == 0 and r["axes_summary"]["max_rest_turn"] == 0
        assert (r["seg"][k] == f + 1).all()


@pytest.mark.parametrize("angle", [5, 60, 90, 150, 175])
@pytest.mark.parametrize("W,dwell", [(1, 0.012), (1, 0.05), (3, 0.1), (8, 0.02), (40, 0.3)])
def test_across_a_rest_the_axes_form_one_chain_with_steps_of_the_chord_over_r(angle, W, dwell):
    q_a = X.fixed_axis((0.0, 1.0, 0.0))
    q_e = X.fixed_axis((np.sin(np.radians(angle)), np.cos(np.radians(angle)), 0.0))
    xyz, q, dw, f = stop_scene(q_a, q_e, dwell)
    r = X.retime_jerk_axes(xyz, q, LIM, dw, W, tick=0.01)
    k = np.flatnonzero(r["rest"])
    Rf = len(k)
    assert Rf >= max(1, int(dwell / 0.01)) and (np.diff(k) == 1).all() and r["R"][f] == Rf and r["first"][f] == k[0]
    assert r["axes_summary"]["n_turning_rests"] == 1 and r["axes_summary"]["min_turn_ticks"] == Rf
    chain = np.concatenate([[k[0] - 1], k, [k[-1] + 1]])
    assert np.array_equal(r["qt"][chain[0]], q_a) and np.array_equal(r["qt"][chain[1]], q_a) and np.array_equal(r["qt"][chain[-1]], q_e)
    lam = np.concatenate([[0.0], np.arange(Rf) / Rf, [1.0]])
    assert np.array_equal(r["lam"][k], lam[1:-1])
    v = q_a[None].astype(np.float64) + (q_e - q_a)[None].astype(np.float64) * lam[:, None]
    ln = np.sqrt((v * v).sum(1))
    step = np.sqrt(float(((q_e - q_a) ** 2).sum())) / Rf
    bound = 16384.0 * step / np.sqrt(ln[:-1] * ln[1:]) + np.sqrt(3.0) + 1e-6
    bound[0] = 0.0   # (the tick in front and the first rest tick both carry q_a)
    d = (r["qt"][chain[1:]] - r["qt"][chain[:-1]]).astype(np.float64)
    chord = np.sqrt((d * d).sum(1))
    assert (chord <= bound).all(), (chord - bound).max()
    assert (r["turn"][chain[1:]] <= (np.floor(bound * bound).astype(np.int64) >> 10)).all()
    assert r["axes_summary"]["max_rest_turn"] == r["turn"][k].max()
    # the steps add up: from q_a to q_e and no further
    assert chord.sum() >= np.sqrt(float(((q_e - q_a) ** 2).sum())) - 1e-9


def test_positions_tags_and_the_profile_are_jerk_refs_own():
    for seed in (1, 3, 5, 7):
        c = X.random_case(seed)
        for W in (1, 6):
            a = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c["dwell"], W, None, c["grid"], c["tool"], c["near_add"], c["tick"], c["tag"])
            b = J.retime_jerk(c["xyz"], c["lim"], c["dwell"], W, None, c["grid"], c["tick"], c["tag"])
            for key in ("time_q", "w_q", "bound", "s_q", "tag", "seg", "rest"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(a["ticks"].view(np.uint32), b["ticks"].view(np.uint32))
            assert a["summary"] == b["summary"] and a["stops"] == b["stops"] and a["jerk"] == b["jerk"]


def test_refusals():
    c = X.random_case(2)
    args = lambda **kw: dict(dict(xyz=c["xyz"], q=c["q"], lim=c["lim"], dwell=c["dwell"], window=3, grid=c["grid"], tool=c["tool"],
                                  near_add=c["near_add"], tick=c["tick"]), **kw)
    X.retime_jerk_axes(**args())
    bad_q = c["q"].copy()
    bad_q[2] = 0
    big_q = c["q"].copy()
    big_q[0, 1] = 16385
    for kw in (dict(q=None), dict(grid=None), dict(tool=None), dict(q=bad_q), dict(q=big_q), dict(near_add=(1 << 30) + 1),
               dict(tool=(np.array([0, -1]), np.array([0, 0]))), dict(tool=(np.array([0, 70000]), np.array([0, 0]))),
               dict(tool=(np.array([0]), np.array([(1 << 30) + 1]))), dict(tool=(np.zeros(65, int), np.zeros(65, int))), dict(window=0)):
        with pytest.raises(ValueError):
            X.retime_jerk_axes(**args(**kw))
