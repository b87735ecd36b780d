"""CPU tests of tests/pose_fit_ref.py, the numpy restatement of wa_grid_pose_fit_trajectory (include/weldacs.h, rules 37 - 39 of the torch
section): the identities the header states, the candidate order on a hand-made case, and the scenes whose figures the GPU tests
(tests/test_gpu_pose_fit.py) compare the device against.

The figures of the scene table were first measured with a prototype built on fit_ref, pose_shortcut_ref, reach_ref and pose_ref; the
restatement written from the header gives the same ones for every scene, and they are recorded here."""
from fractions import Fraction

import numpy as np
import pytest

import clearance_ref as CR
import fit_ref as F
import pose_fit_ref as PF
import pose_shortcut_ref as PS
import reach_ref as RR


def rle(a):
    """[(value, run length)] of a sequence"""
    a = np.asarray(a)
    cut = np.flatnonzero(np.diff(a)) + 1
    start = np.concatenate([[0], cut]).astype(np.int64)
    return [(int(a[s]), int(e - s)) for s, e in zip(start, np.concatenate([cut, [len(a)]]))]


def same_as_fit(r, p, what):
    """identities (a) and (b): everything wa_grid_fit_trajectory returns, bit for bit"""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
    assert r["levels"].tolist() == p["levels"].tolist(), what
    assert (r["rounds"], r["n_cps"], r["n_blocked_first"], r["n_legs"], r["n_legs_at_cap"], r["max_level_used"]) == \
        (p["rounds"], p["n_cps"], p["n_hit_first"], p["n_legs"], p["n_legs_at_cap"], p["max_level_used"]), what
    assert r["final"] == p["final"], what
    assert np.array_equal(bits(r["knots"]), bits(p["knots"])) and np.array_equal(bits(r["cps"]), bits(p["cps"])), what
    assert np.array_equal(bits(r["samples"]), bits(p["samples"])), what
    assert np.array_equal(r["blocked"], p["hits"]) and r["n_blocked"] == p["final"]["n_hit"], what
    assert r["first_blocked"] == p["final"]["first_hit"], what


def identity_cases():
    """(name, grid, dirs, tool, xyz, holds, spacing, n_samples): fit_ref's own scenes, where its loop has rounds to run, with the
    directions and the tool of pose_ref's pillars, and the shortened pose paths"""
    p4 = PF.scene("pillars4")
    out = []
    for name, sc, spacing in (("l_corner", F.l_corner(), 8.0), ("l_corner_long", F.l_corner(long=True), 8.0),
                              ("diagonal_graze", F.diagonal_graze(), 1.0), ("random0", F.random_scene(0), F.RANDOM_SPACING)):
        free, d2, dims, axes, xyz = sc
        out.append((name, (free, d2, dims, axes), p4["dirs"][:5], p4["tool"], xyz, np.arange(len(xyz) - 1) % 5, spacing, 601))
    for name in ("pillars4", "box1"):
        s = PF.scene(name)
        out.append((name, s["grid"], s["dirs"], s["tool"], s["xyz"], s["holds"], 8.0, 601))
    return out


@pytest.mark.parametrize("degree", [2, 3])
def test_identity_a_point_tool_and_every_leg_held(degree):
    for name, grid, dirs, _, xyz, holds, spacing, n in identity_cases():
        held = np.where(np.asarray(holds) >= 0, holds, 0)
        p = F.fit(grid[0], grid[1], grid[2], grid[3], xyz, degree, spacing, 6, n)
        r = PF.fit(grid, dirs, PS.point_tool(), xyz, held, degree, spacing, 6, n)
        same_as_fit(r, p, (name, degree))
        assert r["n_no_candidate"] == 0 and ((r["seg_dir"] >= 0) == (r["blocked"] == 0)).all(), name


@pytest.mark.parametrize("degree", [2, 3])
def test_identity_b_no_leg_held(degree):
    for name, grid, dirs, tool, xyz, holds, spacing, n in identity_cases():
        p = F.fit(grid[0], grid[1], grid[2], grid[3], xyz, degree, spacing, 6, n)
        r = PF.fit(grid, dirs, tool, xyz, np.full(len(xyz) - 1, -1), degree, spacing, 6, n)
        same_as_fit(r, p, (name, degree))
        assert r["n_no_candidate"] == n - 1 and (r["seg_dir"] == -1).all() and r["n_dir_changes"] == 0 and r["max_dir_turn"] == 0, name


def cover_by_slabs(dims, a, b):
    """the voxels whose closed cube the straight segment between the centres of voxels a and b touches, by exact rational slab
    clipping: written without clearance_ref.supercover"""
    nx, ny, _ = dims
    vox = lambda v: np.array([v % nx, (v // nx) % ny, v // (nx * ny)], np.int64)   # noqa: E731
    pa, pb = vox(int(a)), vox(int(b))
    lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
    out = []
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[0], hi[0] + 1):
                t0, t1 = Fraction(0), Fraction(1)
                for c, v in enumerate((x, y, z)):
                    d = int(pb[c] - pa[c])
                    if d == 0:
                        if v != pa[c]:
                            t0, t1 = Fraction(1), Fraction(0)
                        continue
                    e0, e1 = Fraction(2 * (v - int(pa[c])) - 1, 2 * d), Fraction(2 * (v - int(pa[c])) + 1, 2 * d)
                    t0, t1 = max(t0, min(e0, e1)), min(t1, max(e0, e1))
                if t0 <= t1:
                    out.append((z * ny + y) * nx + x)
    return np.array(sorted(out), np.int64)


@pytest.mark.parametrize("name", ["pillars4", "box1", "box2", "wide"])
def test_identity_c_a_direction_is_open_on_the_whole_cover(name):
    s = PF.scene(name)
    r = PF.fitted(name, 3, 8.0, 6, 2001 if name == "pillars4" else 1001)
    free = np.asarray(s["grid"][0]).ravel()
    seen = 0
    for i in np.flatnonzero((r["blocked"] == 0) & (r["seg_dir"] >= 0)):
        cover = cover_by_slabs(s["grid"][2], r["ids"][i], r["ids"][i + 1])
        assert np.array_equal(cover, np.sort(PF.cover_ids(s["grid"][2], r["ids"][i], r["ids"][i + 1]))), i
        assert s["opened"][cover, r["seg_dir"][i]].all() and free[cover].all(), (name, i)
        seen += len(cover) > 1
    assert seen >= 5, "segments that cross voxel boundaries are among them"
    assert (r["seg_dir"][r["blocked"] != 0] == -1).all()


def test_candidate_order_second_candidate_open():
    t = PF.two_leg_case()
    opened = RR.open_dirs(t["grid"], t["dirs"], t["tool"])
    r = PF.fit(t["grid"], t["dirs"], t["tool"], t["xyz"], t["holds"], 3, 8.0, 6, 65, opened)
    cands = [PF.candidates(r["knots"], r["n_cps"], 3, r["owners"], t["holds"], i, r["dt"]) for i in range(64)]
    assert r["rounds"] == 1 and r["n_blocked"] == 0 and r["n_no_candidate"] == 0
    second = [i for i in range(64) if cands[i] == [0, 1] and r["seg_dir"][i] == 1]
    assert second == [39, 40, 41]                         # under the metal voxel: direction 0 is closed there, direction 1 is open
    for i in second:
        cover = PF.cover_ids(t["grid"][2], r["ids"][i], r["ids"][i + 1])
        assert not opened[cover, 0].all() and opened[cover, 1].all()
    assert rle(r["seg_dir"]) == [(0, 39), (1, 3), (0, 6), (1, 16)]
    assert cands[0] == [0, 1] and cands[63] == [1]        # the last spans hold control points of the second leg only
    assert (r["n_dir_changes"], r["max_dir_turn"]) == (3, (4 * 16384 * 16384) >> 10)
    # the other way round both are open along the first leg and the first candidate wins everywhere
    r2 = PF.fit(t["grid"], t["dirs"], t["tool"], t["xyz"], [1, 0], 3, 8.0, 6, 65, opened)
    assert rle(r2["seg_dir"]) == [(1, 48), (0, 16)]


# (scene, samples, holds, blocked segments of the plain fit under the new test, rounds, control points, n_no_candidate)
TABLE = [("pillars4", 2001, [0, -1, -1, 46, 72, -1, -1, -1, 129], 257, 7, 57, 628),
         ("box1", 1001, [0, 4, 4, 0], 17, 4, 22, 0),
         ("box2", 1001, [0, 1, 1], 28, 3, 19, 0),
         ("box3", 1001, [1, 1, 0], 4, 2, 16, 0)]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r[0])
def test_scene_table(row):
    name, n, holds, plain_blocked, rounds, n_cps, n_none = row
    s = PF.scene(name)
    g = s["grid"]
    assert s["holds"].tolist() == holds
    plain = F.fit(g[0], g[1], g[2], g[3], s["xyz"], 3, 8.0, 6, n)
    _, blocked, _ = PF.retest_plain_fit(g, s["opened"], s["xyz"], s["holds"], plain, 3, 8.0)
    assert plain["final"]["n_hit"] == 0 and int(blocked.sum()) == plain_blocked
    r = PF.fitted(name, 3, 8.0, 6, n)
    assert (r["n_blocked_first"], r["rounds"], r["n_cps"], r["n_blocked"], r["n_legs_at_cap"], r["n_no_candidate"]) == \
        (plain_blocked, rounds, n_cps, 0, 0, n_none)
    assert r["final"]["n_hit"] == 0 and r["first_blocked"] == -1
    if name == "pillars4":
        assert r["levels"].tolist() == [0, 0, 0, 0, 5, 5, 6, 6, 6]
        assert rle(r["seg_dir"]) == [(0, 93), (46, 130), (72, 148), (-1, 628), (129, 1001)]
        assert (r["n_dir_changes"], r["max_dir_turn"]) == (2, 373753)


PINNED = {("pillars6", 2): ([(0, 572), (38, 217), (80, 353), (106, 286), (122, 286), (128, 286)], 5, 308749),
          ("pillars6", 3): ([(0, 717), (38, 103), (80, 309), (106, 246), (122, 255), (128, 370)], 5, 308749),
          ("wide", 2): ([(0, 500), (2, 100), (7, 46), (23, 254), (15, 100)], 4, 108238),
          ("wide", 3): ([(0, 546), (2, 81), (23, 283), (15, 90)], 3, 129524)}


@pytest.mark.parametrize("key", sorted(PINNED), ids=lambda k: "%s-%d" % k)
def test_scenes_that_clear_in_round_one_pin_the_directions(key):
    name, degree = key
    runs, changes, turn = PINNED[key]
    r = PF.fitted(name, degree, 8.0, 6, 2001 if name == "pillars6" else 1001)
    assert (r["rounds"], r["n_blocked_first"], r["n_blocked"], r["n_no_candidate"]) == (1, 0, 0, 0)
    assert rle(r["seg_dir"]) == runs and (r["n_dir_changes"], r["max_dir_turn"]) == (changes, turn)


def test_cap_path_does_not_converge():
    r = PF.fitted("pillars4", 2, 8.0, 6, 9)
    assert (r["rounds"], r["n_blocked"], r["n_legs_at_cap"], r["first_blocked"], r["n_blocked_first"]) == (8, 3, 6, 2, 4)
    assert r["blocked"].tolist() == [0, 0, 1, 1, 0, 1, 0, 0] and r["seg_dir"].tolist() == [0, 0, -1, -1, -1, -1, 129, 129]
    assert r["levels"].tolist() == [5, 4, 5, 6, 6, 6, 6, 6, 6] and r["n_no_candidate"] == 1
