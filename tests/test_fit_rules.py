"""The trajectory fit's definition (include/weldacs.h, restated in tests/fit_ref.py) against itself and against geometry, on the CPU:
no GPU, no product code.  The seeded scenes are a CONDITION on the definition, not a measurement: on every committed seed the
reference alone ends with final.n_hit == 0 at max_level 6, and on at least half of them round 1 hits (fit_ref.RANDOM_SEEDS says how
the seeds were chosen)."""
import numpy as np
import pytest

import fit_ref as F


def _hull_ok(r, degree, tol):
    """every sample lies in the bounding box of the D + 1 control points of its knot span, up to the rounding of the evaluation"""
    K, C, S = r["knots"], r["cps"], r["samples"]
    for i in range(len(S)):
        span = F.find_span(K, np.float32(i) * r["dt"])
        box = C[span - degree:span + 1]
        assert (S[i] >= box.min(0) - tol).all() and (S[i] <= box.max(0) + tol).all(), (i, S[i], box)


@pytest.mark.parametrize("degree", [2, 3])
def test_straight_polyline_is_one_round_on_the_line(degree):
    free, d2, dims, axes, xyz = F.straight()
    r = F.fit(free, d2, dims, axes, xyz, degree, 1.0, 6, 601)
    assert r["rounds"] == 1 and r["levels"].tolist() == [0, 0, 0] and r["n_hit_first"] == 0 and r["final"]["n_hit"] == 0
    assert r["n_legs_at_cap"] == 0 and r["max_level_used"] == 0 and r["final"]["n_outside"] == 0
    a, b = xyz[0].astype(np.float64), xyz[-1].astype(np.float64)
    d = (b - a) / np.linalg.norm(b - a)
    off = r["samples"].astype(np.float64) - a
    dist = np.linalg.norm(off - np.outer(off @ d, d), axis=1)
    assert dist.max() < 16 * 2.0 ** -23 * 16          # a few ulps of the largest coordinate
    assert np.array_equal(r["samples"][0], xyz[0]) and np.array_equal(r["samples"][-1], xyz[-1])
    # the zero-length leg contributes one control point: a doubled point of the polygon
    m = F.pieces(xyz, r["levels"], 1.0)
    assert m[1] == 1 and r["n_cps"] == int(m.sum()) + 1 + 2 * (degree - 1)
    assert np.array_equal(r["knots"], np.clip(np.arange(len(r["knots"])) - degree, 0, len(r["knots"]) - 2 * degree - 1).astype(np.float32))
    _hull_ok(r, degree, 1e-5)


def test_l_corner_needs_level_two():
    free, d2, dims, axes, xyz = F.l_corner()
    for degree in (2, 3):
        tr = []
        r = F.fit(free, d2, dims, axes, xyz, degree, 8.0, 6, 601, trace=tr)
        assert r["rounds"] == 3 and r["n_hit_first"] > 0 and r["final"]["n_hit"] == 0 and r["levels"].tolist() == [2, 2]
        assert [t["n_hit"] > 0 for t in tr] == [True, True, False] and r["n_legs_at_cap"] == 0 and r["max_level_used"] == 2
        _hull_ok(r, degree, 1e-5)
        # one level below what it needs: stops at the cap, still hitting
        c = F.fit(free, d2, dims, axes, xyz, degree, 8.0, 1, 601)
        assert c["rounds"] == 2 and c["levels"].tolist() == [1, 1] and c["n_legs_at_cap"] == 2 and c["final"]["n_hit"] > 0
        # max_level 0 is one plain fit
        p = F.fit(free, d2, dims, axes, xyz, degree, 8.0, 0, 601)
        assert p["rounds"] == 1 and p["levels"].tolist() == [0, 0] and p["final"]["n_hit"] == r["n_hit_first"] and p["n_legs_at_cap"] == 2
        assert np.array_equal(p["cps"], F.fit_spline(F.polygon(xyz, F.pieces(xyz, [0, 0], 8.0))[0], degree).cps)


def test_only_the_corner_and_its_blamed_neighbours_rise():
    free, d2, dims, axes, xyz = F.l_corner(long=True)
    r = F.fit(free, d2, dims, axes, xyz, 3, 8.0, 6, 601)
    lv = r["levels"].tolist()
    assert r["rounds"] > 1 and r["final"]["n_hit"] == 0
    assert lv[2] > 0 and lv[3] > 0                     # the two legs that meet at (10, 2)
    assert lv[0] == 0 and lv[-1] == 0                  # the far legs never own a control point near a hit
    assert max(lv) == r["max_level_used"] == 2


def test_diagonal_graze_is_the_documented_limit():
    free, d2, dims, axes, xyz = F.diagonal_graze()
    for ml in (0, 3, 8):
        r = F.fit(free, d2, dims, axes, xyz, 3, 1.0, ml, 601)
        assert r["rounds"] == ml + 1 and r["levels"].tolist() == [ml] and r["n_legs_at_cap"] == 1
        assert r["final"]["n_hit"] == 1 and r["n_hit_first"] == 1     # the one sample pair that steps from (1, 1) to (2, 2)


def test_two_points_zero_length_and_two_samples():
    free, d2, dims, axes, _ = F.straight()
    for degree in (2, 3):
        r = F.fit(free, d2, dims, axes, [[1, 1, 1], [9, 5, 3]], degree, 3.0, 6, 2)
        assert r["rounds"] == 1 and len(r["samples"]) == 2 and r["final"]["n_hit"] == 0
        assert np.array_equal(r["samples"], np.array([[1, 1, 1], [9, 5, 3]], np.float32))
        # a polyline that does not move at all: every leg one piece, the curve a point
        z = F.fit(free, d2, dims, axes, [[4, 4, 2]] * 3, degree, 1.0, 6, 11)
        assert z["rounds"] == 1 and z["n_cps"] == 3 + 2 * (degree - 1)
        assert np.abs(z["samples"] - np.float32([4, 4, 2])).max() <= 4 * 2.0 ** -22   # (the basis sums to 1 up to its fp32 rounding)
        assert z["final"]["min_d2"] == F.CR.D2_NONE
    # two samples whose straight cover crosses the metal: no level changes the two end voxels
    free, d2, dims, axes, xyz = F.l_corner()
    free = free.copy()
    free[(np.arange(256) // 16 >= 3) & (np.arange(256) % 16 <= 9) & (np.arange(256) // 16 <= 9) & (np.arange(256) % 16 >= 3)] = 0
    d2 = F.CR.edt_separable(free, *dims)
    r = F.fit(free, d2, dims, axes, xyz, 3, 8.0, 2, 2)
    assert r["rounds"] == 3 and r["final"]["n_hit"] == 1 and r["n_legs_at_cap"] == 2 and r["levels"].tolist() == [2, 2]


_results = {}


def _scene_result(seed):
    if seed not in _results:
        sc = F.random_scene(seed)
        assert sc is not None, "seed %d: end points not connected" % seed
        _results[seed] = (sc, F.fit(*sc, 3, F.RANDOM_SPACING, 6, F.RANDOM_SAMPLES))
    return _results[seed]


@pytest.mark.parametrize("seed", F.RANDOM_SEEDS)
def test_seeded_scene_reaches_zero(seed):
    (free, d2, dims, axes, xyz), r = _scene_result(seed)
    assert 24 <= dims[0] <= 40 and 0.05 <= 1.0 - free.mean() <= 0.15 + 0.01
    assert r["final"]["n_hit"] == 0 and r["n_legs_at_cap"] == 0 and r["rounds"] < F.MAX_ROUNDS
    assert r["rounds"] == 1 or r["n_hit_first"] > 0
    _hull_ok(r, 3, 1e-4)


def test_seed_list_makes_the_loop_work():
    assert len(F.RANDOM_SEEDS) >= 20 and len(set(F.RANDOM_SEEDS)) == len(F.RANDOM_SEEDS)
    worked = sum(_scene_result(s)[1]["n_hit_first"] > 0 for s in F.RANDOM_SEEDS)
    assert 2 * worked >= len(F.RANDOM_SEEDS), worked


# ------------------------------------------------------------------ polylines of many legs (fit_ref.many_legs_scene)
# What tests/test_gpu_fit.py compares on the device must exercise what it is there for: hits in round 1, a second round, raised legs
# behind the first block of 256 legs (behind the first trip of 256 blocks for the large ones) and at the very end, legs at the cap, and
# piece counts that differ (a constant m_k would hide a shifted prefix).
MANY = [(n, d) for n in F.BLOCK_LEGS for d in (2, 3)] + [(n, 3) for n in F.PASS_LEGS] + [("zero_tail", 3), ("long_legs", 3)]


@pytest.mark.parametrize("case", MANY, ids=lambda c: "%s-%d" % c)
def test_many_legs_scene_exercises_the_scan(case):
    name, degree = case
    (free, d2, dims, axes, xyz), (_, spacing, max_level, n_samples), r = F.many_legs_case(name, degree)
    n_legs = len(xyz) - 1
    print("[fit] many legs %s, degree %d: %d legs, %d samples, %d rounds, %d control points, reference %.1f s of CPU"
          % (name, degree, n_legs, n_samples, r["rounds"], r["n_cps"], r["cpu_seconds"]))
    assert n_legs == (name if isinstance(name, int) else n_legs) == r["n_legs"] and dims[0] in (48, 64) and int((free == 0).sum()) > 0
    assert n_samples >= n_legs or n_legs < 65535                # large scenes: a sample segment stays local
    raised = np.flatnonzero(r["levels"] > 0)
    assert r["n_hit_first"] > 0 and r["rounds"] >= 2 and r["rounds"] < F.MAX_ROUNDS
    assert len(raised) > 0 and raised.max() >= n_legs - 64      # one in the last 64 legs
    if n_legs > 256:
        assert (raised >= 256).any()
    if n_legs > 65536:
        assert (raised >= 65536).any()
    if n_legs > 131072:
        assert (raised >= 131072).any()
    assert r["n_legs_at_cap"] > 0 and r["max_level_used"] == max_level
    m = F.pieces(xyz, np.zeros(n_legs, np.int64), spacing)
    # m_k = 1, 2, 3 with shares of about 0.46, 0.46, 0.08: neighbours differ with probability 1 - sum p^2 = 0.57 (+- 0.06 at 63 legs)
    assert len(np.unique(m)) >= 3 and (np.diff(m[:300]) != 0).mean() > 0.3
    zero = F.leg_lengths(xyz) == 0.0
    if name == "zero_tail":
        assert zero[300:].all() and (m[300:] == 1).all() and r["n_cps"] >= n_legs
    else:
        assert 0.01 <= zero.mean() <= 0.035 or n_legs < 1000     # about 2 % ...
        if n_legs >= 1000:
            assert (zero[1:] & zero[:-1]).any()                  # ... some of them in a row
    if name == "long_legs":
        assert (m >= 400).sum() == 7 and (m >= 1000).sum() >= 4 and np.median(m) <= 2   # (a long leg round a turn is a shorter chord)
    assert r["cpu_seconds"] < 60.0
