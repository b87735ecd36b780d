"""The restatements of the timing calls (tests/retime_ref.py, stops_ref.py, jerk_ref.py; no product code) held against Python-integer
forms of the header's rules on the scenes of tests/magnitude_ref.py: long paths, prefix sums of U past 2^53 and past 2^64, caps
saturated at 2^61 and caps of 0 and 1 quantum, sums and durations just under 2^61.  The numpy restatements are what the device is held
against bit for bit; here they are shown to be right where the numbers are large.

jerk_ref.window_means built its prefix sums in float64 (a Python 0 in front of a uint64 array) until it was held against this file:
every scene whose prefix sums pass 2^53 fails test_window_means_are_exact with that version."""
import numpy as np
import pytest

import jerk_ref as J
import magnitude_ref as M
import retime_ref as R

CAP = R.CAP_INF


def exact_window_means(U, W, length_q):
    """rule 53 with Python integers only: a running sum of the last W of 0 .. 0, U_0 .. U_(n_u - 1), length_q .. length_q"""
    U = [int(u) for u in U.tolist()]
    n_u = len(U)
    at = lambda k: 0 if k < 0 else (length_q if k >= n_u else U[k])
    out, s = [], 0
    for k in range(n_u + W - 1):
        s += at(k) - at(k - W)
        out.append(s // W)
    return out


def recurrence(C, A, D):
    """rule 3, literally, with Python integers: F_i = min(C_i, F_(i-1) + A_(i-1)), B_i = min(F_i, B_(i+1) + D_i)"""
    C, A, D = ([int(x) for x in v.tolist()] for v in (C, A, D))
    n = len(C)
    F = [C[0]] + [0] * (n - 1)
    for i in range(1, n):
        F[i] = min(C[i], F[i - 1] + A[i - 1])
    B = F[:]
    for i in range(n - 2, -1, -1):
        B[i] = min(F[i], B[i + 1] + D[i])
    return F, B


def check_profile(r, n_ends):
    """the inequalities of test_retime_rules._check_profile, with Python integers where two values near 2^61 meet; n_ends: the kind-0
    samples (the two end points and the samples of every stop)"""
    C, B, A, D = ([int(x) for x in r[k].tolist()] for k in ("C", "w_q", "A", "D"))
    n = len(C)
    assert all(0 <= B[i] <= C[i] <= CAP for i in range(n))
    assert all(B[i + 1] - B[i] <= A[i] and B[i] - B[i + 1] <= D[i] for i in range(n - 1))
    assert ((r["bound"] & 7) != 0).all()                             # on a cap or on a ramp everywhere
    t = [int(x) for x in r["time_q"].tolist()]
    assert t[0] == 0 and all(t[i] <= t[i + 1] for i in range(n - 1)) and t[-1] == r["summary"]["time_q"] < CAP
    assert sum(r["summary"]["n_bound"]) == r["summary"]["n"] == n and r["summary"]["n_bound"][0] == n_ends


@pytest.mark.parametrize("name", list(M.SCENES))
def test_window_means_are_exact(name):
    r = M.reference(name)
    W, length_q = r["jerk"]["window"], r["summary"]["length_q"]
    assert r["s_q"].dtype == np.int64 and r["s_q"].tolist() == exact_window_means(r["U"], W, length_q)


@pytest.mark.parametrize("name", list(M.SCENES))
def test_the_jerk_bound_and_the_end_values(name):
    r = M.reference(name)
    j = r["jerk"]
    assert j["max_d3"] <= 2 * j["in_max_d2"] // j["window"] + 4, j
    assert j["n_back"] == 0 and int(r["s_q"][0]) == 0 and int(r["s_q"][-1]) == r["summary"]["length_q"]
    assert j["n_ticks"] == j["n_in"] + j["window"] - 1 == len(r["s_q"]) == len(r["ticks"])
    d1 = [b - a for a, b in zip(r["s_q"][:5000].tolist(), r["s_q"][1:5001].tolist())]   # (the summary's own differences, in Python integers)
    assert max(d1) <= j["max_d1"] and min(d1) >= 0


@pytest.mark.parametrize("name", M.SMALL)
def test_the_array_form_is_the_scalar_form(name):
    """(not on third_level: the scalar form adds W = 64 values for each of 4 million ticks; test_window_means_are_exact holds its s_q
    against a running sum)"""
    xyz, lim, tick, W, dwell, v_limit, seg_tag = M.scene(name)
    r = M.reference(name)
    s_q, segs, rests, pos, tags = J.retime_jerk_scalar(xyz, lim, dwell, W, v_limit, None, tick, seg_tag)
    assert s_q == r["s_q"].tolist() and segs == r["seg"].tolist() and rests == r["rest"].tolist()
    assert pos.tobytes() == r["ticks"].tobytes()
    assert tags is None and r["tag"] is None if seg_tag is None else tags == r["tag"].tolist()


@pytest.mark.parametrize("name", list(M.SCENES))
def test_the_lowered_profile_is_the_recurrence(name):
    """the profile under the lowered caps of rule 49 (retime_jerk's C), stops included"""
    r = M.reference(name)
    F, B = recurrence(r["C"], r["A"], r["D"])
    assert B == r["w_q"].tolist()
    Fs, Bs = R.passes_sequential(r["C"], r["A"], r["D"])
    assert Fs.tolist() == F and Bs.tolist() == B
    check_profile(r, 2 + r["stops"]["n_stop_samples"])


@pytest.mark.parametrize("stops", [False, True])
@pytest.mark.parametrize("name", M.PROFILE_SCENES)
def test_retime_and_stops_are_the_recurrence(name, stops):
    r = M.profile_reference(name, stops)
    F, B = recurrence(r["C"], r["A"], r["D"])
    assert F == r["F"].tolist() and B == r["w_q"].tolist()
    Fs, Bs = R.passes_sequential(r["C"], r["A"], r["D"])
    assert Fs.tolist() == F and Bs.tolist() == B
    check_profile(r, 2 + (r["stops"]["n_stop_samples"] if stops else 0))
    assert len(r["ticks"]) == r["summary"]["n_ticks"]


def test_the_pairs_stand_on_both_sides_of_their_refusals():
    xyz, lim, tick, _, _, _, _ = M.scene("wrap_w127")
    assert M.accepted(lambda: J.retime_jerk(xyz, lim, None, 127, tick=tick, want_ticks=False))
    assert not M.accepted(lambda: J.retime_jerk(xyz, lim, None, 128, tick=tick, want_ticks=False))
    for name in ("saturated_acc", "saturated_dec", "saturated_2049"):
        xyz, lim, tick, W, _, _, _ = M.scene(name)
        M.reference(name)
        over = dict(lim, **{k: 2.0 ** 20 for k in ("acc", "dec") if lim[k] == M.ACC_LAST})
        assert over != lim
        for call in (lambda l: R.retime(xyz, l, tick=tick, want_ticks=False), lambda l: J.retime_jerk(xyz, l, None, W, tick=tick, want_ticks=False)):
            assert M.accepted(lambda: call(lim)) and not M.accepted(lambda: call(over)), name
    for pair in (M.extended_dwell_pair(), M.duration_pair(1), M.duration_pair(M.PAIR_W)):
        good, bad = pair[2], pair[3]
        k = np.flatnonzero(good >= 0)
        assert len(k) == 1 and bad[k[0]] == np.nextafter(good[k[0]], np.inf)   # one step apart
