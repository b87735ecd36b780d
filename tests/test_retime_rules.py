"""CPU checks of the re-timing definition itself (tests/retime_ref.py; no product code): the closed forms against the recurrences, the
inequalities a speed profile must satisfy, the on-cap-or-on-ramp property, analytic profiles, each kind of cap, and the ticks."""
import numpy as np
import pytest

import clearance_ref as CR
import retime_ref as R

Q = R.Q


def _check_profile(r):
    C, B, A, D = r["C"], r["w_q"], r["A"], r["D"]
    assert (B <= C).all() and (B >= 0).all()
    assert (B[1:] - B[:-1] <= A).all() and (B[:-1] - B[1:] <= D).all()
    assert ((r["bound"] & 7) != 0).all()                      # on a cap or on a ramp everywhere
    assert (np.diff(r["time_q"]) >= 0).all() and r["time_q"][0] == 0 and r["time_q"][-1] == r["summary"]["time_q"]
    assert sum(r["summary"]["n_bound"]) == r["summary"]["n"] and r["summary"]["n_bound"][0] == 2


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_closed_forms_equal_the_recurrences(seed):
    grid, xyz, lim, v_limit, tick = R.random_scene(seed)
    for g in (grid, None):
        r = R.retime(xyz, lim, v_limit, g, tick)
        F, B = R.passes_sequential(r["C"], r["A"], r["D"])
        assert np.array_equal(F, r["F"]) and np.array_equal(B, r["w_q"])
        _check_profile(r)


def test_every_kind_binds_on_at_least_half_of_the_seeded_scenes():
    seen = np.zeros(4, int)
    for seed in R.RANDOM_SEEDS:
        grid, xyz, lim, v_limit, tick = R.random_scene(seed)
        r = R.retime(xyz, lim, v_limit, grid, tick, want_ticks=False)
        on = (r["bound"] & 1).astype(bool)
        for k in range(4):
            seen[k] += bool((on & (r["kind"] == k)).any())
    assert (2 * seen >= len(R.RANDOM_SEEDS)).all(), seen


def test_axis_lookup_is_the_one_of_the_clearance_reference():
    rs = np.random.RandomState(11)
    for c in (np.arange(20, dtype=np.float32), np.sort(rs.uniform(-1, 1, 17)).astype(np.float32),
              np.array([0, 1, 2, 2, 3, 3.5], np.float32)):
        p = np.concatenate([rs.uniform(c.min() - 1, c.max() + 1, 300), c, (c[1:] + c[:-1]) / 2, [np.nan]]).astype(np.float32)
        j, out = R.axis_nodes(c, p)
        for k in range(len(p)):
            assert (int(j[k]), bool(out[k])) == CR.axis_node(c, p[k])


def _spacing_error(h, v_max, acc, dec):
    """What sampling every h units can add to an analytic duration.  The discrete profile differs from the continuous one only in the
    two samples around each of its two kinks, where it is lower by at most the ramp's rise over one spacing, 2 * max(acc, dec) * h in
    squared speed; over a stretch of 2 h at a speed within that of v_max this costs at most 2 h * (1 / v_lo - 1 / v_max) with
    v_lo^2 = v_max^2 - 2 * max(acc, dec) * h, per kink; the first and last segments (from and to rest) are exact for constant acceleration."""
    a = max(acc, dec)
    v_lo = np.sqrt(v_max * v_max - 2 * a * h)
    return 2 * (2 * h) * (1 / v_lo - 1 / v_max)


def test_straight_line_trapezoid_and_triangle():
    v, acc, dec, length = 0.5, 1.0, 2.0, 2.0
    for n in (1001, 100001):
        r = R.retime(R.line(n, length), R.limits(v_max=v, acc=acc, dec=dec))
        _check_profile(r)
        want = length / v + v / (2 * acc) + v / (2 * dec)                        # 4.375 s
        slack = (n + 1) / Q + _spacing_error(length / (n - 1), v, acc, dec)
        assert abs(r["summary"]["time_q"] / Q - want) <= slack, (n, r["summary"]["time_q"] / Q, want, slack)
        assert r["summary"]["peak_w_q"] == int(v * v * Q)
    length = 0.1                                                                 # too short to reach v_max: a triangle
    for n in (1001, 20001):
        r = R.retime(R.line(n, length), R.limits(v_max=v, acc=acc, dec=dec))
        _check_profile(r)
        wp = 2 * length * acc * dec / (acc + dec)
        want = np.sqrt(wp) / acc + np.sqrt(wp) / dec
        h = length / (n - 1)
        # one kink, at the peak: the profile is below the continuous one by at most 2 max(acc, dec) h over two spacings around it
        v_lo = np.sqrt(wp - 2 * max(acc, dec) * h)
        slack = (n + 1) / Q + 2 * h * (1 / v_lo - 1 / np.sqrt(wp))
        assert abs(r["summary"]["time_q"] / Q - want) <= slack, (n, r["summary"]["time_q"] / Q, want, slack)
        assert r["summary"]["peak_w_q"] < int(v * v * Q)


def test_two_points_travel_rest_to_rest():
    xyz = np.array([[0, 0, 0], [1, 2, 2]], np.float32)                           # 3 units
    r = R.retime(xyz, R.limits(v_max=9, acc=1, dec=3), tick=0.125)
    wp = 2 * 3 * 1 * 3 / 4
    assert r["summary"]["n_triangle"] == 1 and r["w_q"].tolist() == [0, 0] and r["bound"].tolist() == [1, 1]
    assert abs(r["summary"]["time_q"] / Q - (np.sqrt(wp) + np.sqrt(wp) / 3)) < 2.0 / Q
    t = r["ticks"]
    assert np.array_equal(t[0], xyz[0]) and np.array_equal(t[-1], xyz[1]) and len(t) == r["summary"]["n_ticks"]
    s = np.linalg.norm(t.astype(np.float64) - xyz[0], axis=1)
    assert (np.diff(s) >= 0).all()
    k = np.arange(len(t) - 1) * 0.125
    up = k <= np.sqrt(wp)
    assert np.allclose(s[:-1][up], 0.5 * k[up] ** 2, atol=1e-6)                  # the acceleration leg of the triangle


def test_repeated_points_take_no_time():
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0]], np.float32)
    r = R.retime(xyz, R.limits(v_max=0.5, acc=1, dec=2), tick=0.05)
    _check_profile(r)
    assert r["L"].tolist() == [0, Q, 0, 0, Q, 0] and r["T"][[0, 2, 3, 5]].tolist() == [0, 0, 0, 0]
    assert (r["w_q"][2:5] == r["w_q"][2]).all()
    assert np.array_equal(r["ticks"][0], xyz[0]) and np.array_equal(r["ticks"][-1], xyz[-1])
    r = R.retime(np.zeros((5, 3), np.float32), R.limits())
    assert r["summary"]["time_q"] == 0 and r["summary"]["n_ticks"] == 1 and len(r["ticks"]) == 1


def test_a_corner_slows_to_the_curvature_cap():
    xyz = R.right_angle(200, 1.0)
    corner = 200
    lim = R.limits(v_max=1, acc=2, dec=2, a_lat=0.5)
    r = R.retime(xyz, lim)
    _check_profile(r)
    # Menger curvature of the corner sample: legs of h = 1/200 at a right angle, circumradius h / sqrt 2
    h = 1.0 / 200
    cap = 0.5 * h / np.sqrt(2.0)
    assert r["kind"][corner] == R.KIND_CURV and r["bound"][corner] & 1
    assert abs(r["w_q"][corner] / Q - cap) < 1e-6 * cap + 2.0 / Q
    free = R.retime(xyz, R.limits(v_max=1, acc=2, dec=2, a_lat=np.inf))
    assert free["kind"][corner] == R.KIND_VMAX and free["w_q"][corner] == Q and free["summary"]["time_q"] < r["summary"]["time_q"]
    assert np.array_equal(R.retime(xyz, R.limits(v_max=1, acc=2, dec=2, a_lat=0.0))["w_q"], free["w_q"])
    r = R.retime(R.helix(4001), R.limits(v_max=3, acc=5, dec=5, a_lat=0.4))
    b = 0.05 / (2 * np.pi)
    want = 0.4 * (0.25 + b * b) / 0.5                                            # a_lat over the helix's curvature
    mid = r["w_q"][1000:3000] / Q
    # three samples a chord h apart bulge by h^2 / (2 R) from their chord; rounding to fp32 moves each sample by up to sqrt(3) half ulps of
    # 0.5 (2^-25 each axis), which moves the bulge by up to twice that: the relative error of the curvature the samples show
    hh = 2 * np.pi * 2 * np.sqrt(0.25 + b * b) / 4000
    rtol = 2 * np.sqrt(3.0) * 2.0 ** -25 / (hh * hh / (2 * (0.25 + b * b) / 0.5)) + 1e-4
    assert np.allclose(mid, want, rtol=rtol), rtol


def test_near_the_metal_the_clearance_cap_binds():
    grid, xyz = R.slab_scene()
    lim = R.limits(v_max=2.0, acc=4.0, dec=4.0, v_near=0.25, near_d2=9)
    r = R.retime(xyz, lim, grid=grid)
    _check_profile(r)
    sd, n_out = R.sample_d2(grid, xyz)
    ids, sd2, _, _ = CR.clearance(grid[0], grid[1], *grid[2], *grid[3], xyz)
    assert np.array_equal(sd, sd2) and n_out == 0
    near = sd <= 9
    assert near.any() and not near.all()
    assert (r["kind"][1:-1] == np.where(near, R.KIND_NEAR, R.KIND_VMAX)[1:-1]).all()
    assert (r["w_q"][near] <= int(0.0625 * Q)).all() and (r["w_q"][near] == int(0.0625 * Q)).sum() > near.sum() // 2
    free = R.retime(xyz, lim)
    assert free["summary"]["n_bound"][3] == 0 and free["w_q"].max() == 4 * Q and free["summary"]["time_q"] < r["summary"]["time_q"]
    assert (free["w_q"][near][5:-5] > int(0.0625 * Q)).all()


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:12])
def test_ticks_lie_on_their_segments_and_never_go_back(seed):
    grid, xyz, lim, v_limit, tick = R.random_scene(seed)
    r = R.retime(xyz, lim, v_limit, grid, tick)
    t = r["ticks"].astype(np.float64)
    p = xyz.astype(np.float64)
    n = len(xyz)
    assert len(t) == r["summary"]["n_ticks"]
    assert np.array_equal(r["ticks"][0], xyz[0]) and np.array_equal(r["ticks"][-1], xyz[-1])
    taus = np.minimum(np.arange(len(t), dtype=np.int64) * r["tick_q"], r["summary"]["time_q"])
    i = np.searchsorted(r["time_q"][:n - 1], taus, side="right") - 1
    a, b = p[i], p[i + 1]
    ab = b - a
    len2 = (ab * ab).sum(1)
    lam = np.where(len2 > 0, ((t - a) * ab).sum(1) / np.where(len2 > 0, len2, 1), 0.0)
    off = np.linalg.norm(t - (a + ab * lam[:, None]), axis=1)
    scale = np.abs(p).max()
    assert (off <= 4 * scale * 2.0 ** -24).all() and (lam >= -1e-6).all() and (lam <= 1 + 1e-6).all()
    cum = np.concatenate([[0.0], np.cumsum(r["ds"])])
    arc = cum[i] + np.clip(lam, 0, 1) * r["ds"][i]
    assert (np.diff(arc) >= -8 * scale * 2.0 ** -24).all()
    fine = R.retime(xyz, lim, v_limit, grid, tick / 10)
    assert np.array_equal(fine["time_q"], r["time_q"]) and np.array_equal(fine["w_q"], r["w_q"])
    assert fine["summary"]["n_ticks"] >= 10 * (r["summary"]["n_ticks"] - 2)


def test_refusals():
    xyz = R.line(11)
    ok = R.limits()
    for bad in (dict(v_max=0), dict(v_max=np.inf), dict(acc=0), dict(acc=np.nan), dict(dec=-1), dict(a_lat=-1), dict(a_lat=np.nan),
                dict(acc=1e12), dict(dec=1e12)):                               # (the last two: the sum of A / of D alone reaches 2^61)
        with pytest.raises(ValueError):
            R.retime(xyz, dict(ok, **bad))
    for tick in (0.0, -1.0, np.nan, np.inf, 2.0 ** -32, 1e10):
        with pytest.raises(ValueError):
            R.retime(xyz, ok, tick=tick)
    with pytest.raises(ValueError):
        R.retime(xyz[:1], ok)
    far = xyz.copy()
    far[3, 0] = 3e38
    with pytest.raises(ValueError):
        R.retime(far, ok)
    with pytest.raises(ValueError):
        R.retime(xyz, ok, v_limit=np.zeros(11, np.float32))
    r = R.retime(R.line(1001), R.limits(v_max=0.5, acc=1, dec=2), tick=2.0 ** -30)
    assert r["ticks"] is None and r["summary"]["n_ticks"] == r["summary"]["time_q"] + 1 > R.MAX_TICKS
