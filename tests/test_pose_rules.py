"""CPU tests of tests/pose_ref.py, the numpy restatement of the exact pose paths (include/weldacs.h, rules 17 - 23 of the torch section):
against an explicit-state queue search, against the reductions the definition implies, on the two-pillar scene of DESIGN 4t, on a tie
scene worked out by hand, and that the scenes of tests/test_gpu_pose.py decide something."""
import numpy as np
import pytest

import geodesic_ref as GR
import pose_ref as PR
import reach_ref as RR
import torch_ref as TR


def small_scene(seed):
    """a seeded scene of at most 10^3 voxels with boxes and speckles, K <= 9 directions, a short rod"""
    rs = np.random.RandomState(9100 + seed)
    dims = tuple(int(v) for v in rs.randint(3, 11, 3))
    free = (rs.uniform(size=dims[::-1]) > 0.03).astype(np.uint8)
    for _ in range(int(rs.randint(0, 3))):
        lo = [int(rs.randint(0, m)) for m in dims]
        sz = [int(rs.randint(1, 4)) for _ in dims]
        free[lo[2]:lo[2] + sz[2], lo[1]:lo[1] + sz[1], lo[0]:lo[0] + sz[0]] = 0
    K = int(rs.randint(1, 10))
    dirs = rs.normal(size=(K, 3)).astype(np.float32)
    tool = TR.rod(int(rs.randint(1, 5)), int(rs.randint(16, 64)), int(rs.randint(0, 3)))
    max_turn = int(rs.choice([-1, 0, 150000, 300000, 500000, 700000]))
    sc = PR.Scene(TR.make_grid(free, dims), dirs, tool, max_turn)
    some = np.flatnonzero(sc.opened.any(1))
    src = int(rs.choice(some if len(some) and seed % 4 else np.flatnonzero(sc.free)))   # (every fourth: any free voxel, the seed may be empty)
    pin = int(rs.choice(np.flatnonzero(sc.opened[src]))) if sc.opened[src].any() and seed % 3 else int(rs.randint(-1, K))
    return sc, src, pin


@pytest.mark.parametrize("seed", range(10))
def test_restatement_against_a_queue_over_explicit_states(seed):
    sc, src, pin = small_scene(seed)
    for p in sorted({-1, pin}):
        state, hops = sc.levels(src, p)
        want = sc.queue_levels(src, p)
        assert np.array_equal(state, want), (seed, p)
        big = np.where(want >= 0, want, 1 << 30).min(0)
        assert np.array_equal(hops, np.where(big < (1 << 30), big, -1))
        assert (state[:, ~sc.free] < 0).all() and (state.T[~sc.opened] < 0).all()
        # an empty seed reaches nothing, the source included
        if not sc.seed(src, p).any():
            assert (state < 0).all() and (hops < 0).all()


def test_the_small_scenes_decide_something():
    facts = []
    for seed in range(10):
        sc, src, pin = small_scene(seed)
        state, _ = sc.levels(src, pin)
        facts.append((int((state >= 0).sum()), int(((state < 0).T & sc.opened).sum())))
    print(facts)
    assert sum(1 for r, u in facts if r > 0 and u > 0) >= 4, facts
    assert sum(1 for r, u in facts if r > 50) >= 7, facts


@pytest.fixture(scope="module")
def box():
    grid, dirs, tool = RR.box_scene(1, 14)
    return grid, dirs, tool, PR.spread_points(grid, 4)


def test_reduction_no_turn_limit_is_the_fit_grid(box):
    grid, dirs, tool, pts = box
    sc = PR.Scene(grid, dirs, tool, -1)
    fit = RR.fit(grid, dirs, tool, 1)
    assert (fit != grid[0]).any()                                  # the fit grid differs from the grid
    pts = [p for p in pts if fit[p]]
    assert len(pts) >= 3
    for p in pts:
        assert np.array_equal(sc.levels(p)[1], GR.field(fit, grid[2], p))
    assert np.array_equal(sc.matrix(pts), GR.matrix(fit, grid[2], pts))


@pytest.mark.parametrize("max_turn", [-1, 0, 70000])
def test_reduction_one_direction_is_the_fit_grid(box, max_turn):
    grid, dirs, tool, pts = box
    d1 = dirs[3:4]
    sc = PR.Scene(grid, d1, tool, max_turn)
    fit = RR.fit(grid, d1, tool, 1)
    assert (fit != grid[0]).any()
    for p in pts:
        if fit[p]:
            assert np.array_equal(sc.levels(p)[1], GR.field(fit, grid[2], p))
        else:
            assert (sc.levels(p)[1] < 0).all()                     # a free source without an open direction: an empty seed


@pytest.mark.parametrize("max_turn", [-1, 0, 300000])
def test_reduction_no_obstacles_is_the_grid(max_turn):
    dims = (7, 5, 6)
    grid = TR.make_grid(np.ones(int(np.prod(dims)), np.uint8), dims)
    sc = PR.Scene(grid, TR.fib_dirs(7, 2.0), TR.rod(4, 80, 2), max_turn)
    assert sc.opened.all()
    for p in (0, 100, 209):
        assert np.array_equal(sc.levels(p)[1], GR.field(grid[0], dims, p))
        assert np.array_equal(sc.levels(p, 4)[1], GR.field(grid[0], dims, p))


def test_reduction_matrix_is_symmetric_with_the_same_pins():
    for seed in (0, 2):
        c = PR.box_case(seed)
        sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
        m = sc.matrix(c["points"], c["pins"])
        assert np.array_equal(m, m.T) and (m < 0).any() and (m > 0).any()
        m = sc.matrix(c["points"])
        assert np.array_equal(m, m.T)


PILLARS = {4: (9, 9, 13, -1, -1), 6: (11, 11, 11, 11, 13)}   # fit grid, then max_turn -1, 150 000, 80 000, 30 000


@pytest.fixture(scope="module")
def pillar_scenes():
    out = {}
    for gap in PILLARS:
        p = PR.pillars(gap)
        out[gap] = (p, PR.Scene(p["grid"], p["dirs"], p["tool"], -1))
    return out


@pytest.mark.parametrize("gap", sorted(PILLARS))
def test_pillars_give_the_table_of_the_design(pillar_scenes, gap):
    p, sc = pillar_scenes[gap]
    assert p["grid"][2] == (12 + gap, 21, 21) and len(p["dirs"]) == 130
    fit = RR.fit(p["grid"], p["dirs"], p["tool"], 1, count=sc.opened.sum(1))
    got = [int(GR.field(fit, p["grid"][2], p["start"])[p["end"]])]
    deepest = []
    for mt in (-1, 150000, 80000, 30000):
        s = sc.with_turn(mt)
        state, hops = s.levels(p["start"])
        got.append(int(hops[p["end"]]))
        deepest.append(int(state.max()))
        D, ids, ks = s.path(p["start"], p["end"])
        assert D == got[-1]
        if D >= 0:
            s.check_path(ids, ks, p["start"], p["end"], -1, -1, D)
    print(gap, got, deepest)
    assert tuple(got) == PILLARS[gap]
    if gap == 4:
        assert deepest[1] == 34          # max_turn 150 000: deeper than one block of 32 launches


def test_every_path_keeps_its_ends_pins_turns_and_length():
    for c in (PR.box_case(0), PR.wide_case()):
        sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
        pts, pins = c["points"], c["pins"]
        n_paths = 0
        for i, (s, ps) in enumerate(zip(pts, pins)):
            for j, (e, pe) in enumerate(zip(pts, pins)):
                D, ids, ks = sc.path(s, e, ps, pe)
                assert D == sc.hops_to(s, ps, e, pe)
                if D < 0:
                    assert ids is None and ks is None
                    continue
                sc.check_path(ids, ks, s, e, ps, pe, D)
                n_paths += 1
                if i == j:
                    assert D == 0 and len(ids) == 1
        assert n_paths > len(pts)


def test_tie_scene_neighbour_order_and_lowest_direction():
    """2 x 2 x 2 without obstacles, directions +x, +y, -x: U(0, 1) = U(1, 2) = 2^19, U(0, 2) = 2^20, so with max_turn = 600 000 direction 0
    reaches 2 only through 1.  From (voxel 0, direction 0) to (voxel 7, direction 2): 3 hops.  Walking back from (7, 2): -x comes first
    of the three neighbours at level 2, voxel 6, where directions 1 and 2 both have level 2 and are within the limit of 2 -- the lowest,
    1; from (6, 1): no -x, +x is voxel 7, -y is voxel 4, whose directions 0 and 1 have level 1 -- 0; then the start."""
    grid = TR.make_grid(np.ones(8, np.uint8), (2, 2, 2))
    dirs = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0]], np.float32)
    q = TR.quantise_all(dirs)
    assert int(TR.turn(q[0], q[1])) == 1 << 19 and int(TR.turn(q[1], q[2])) == 1 << 19 and int(TR.turn(q[0], q[2])) == 1 << 20
    sc = PR.Scene(grid, dirs, TR.rod(2, 16, 0), 600000)
    state, hops = sc.levels(0, 0)
    assert state[:, 6].tolist() == [2, 2, 2] and state[:, 4].tolist() == [1, 1, 3] and hops.tolist() == [0, 1, 1, 2, 1, 2, 2, 3]
    D, ids, ks = sc.path(0, 7, 0, 2)
    assert D == 3 and ids.tolist() == [0, 4, 6, 7] and ks.tolist() == [0, 0, 1, 2]
    # without the end pin the end state is the lowest direction at level 3, and the walk never turns
    D, ids, ks = sc.path(0, 7, 0, -1)
    assert D == 3 and ids.tolist() == [0, 4, 6, 7] and ks.tolist() == [0, 0, 0, 0]
    # a turn limit below 2^19 leaves direction 2 out of reach of a start pinned to 0
    assert sc.with_turn(500000).path(0, 7, 0, 2)[0] == -1


# ---- the scenes of tests/test_gpu_pose.py decide something
@pytest.mark.parametrize("name", ["box0", "box1", "box2", "box3", "tunnel", "wide"])
def test_gpu_scenes_are_not_degenerate(name):
    c = PR.box_case(int(name[3])) if name.startswith("box") else PR.tunnel_case() if name == "tunnel" else PR.wide_case()
    unreached, later, deepest, hops = PR.first_field_facts(c)
    print(name, unreached, later, deepest, hops)
    assert unreached > 0 and later > 0
    assert (hops[1:] > 0).any()
    if name == "tunnel":
        assert deepest > 64 and hops[1] > 0          # start and end stay connected
    if name == "wide":
        assert deepest > 64 and c["grid"][2] == (70, 9, 7) and len(c["dirs"]) == 33
    if name.startswith("box"):
        assert len(c["dirs"]) in (5, 16, 33) and c["grid"][2] == (24, 24, 24) and len(c["points"]) == 6


def test_gpu_pillars_are_not_degenerate(pillar_scenes):
    p, sc = pillar_scenes[4]
    fit = RR.fit(p["grid"], p["dirs"], p["tool"], 1, count=sc.opened.sum(1))
    gh = GR.field(fit, p["grid"][2], p["start"])
    s = sc.with_turn(80000)
    state, hops = s.levels(p["start"])
    assert ((state < 0).T & s.opened).any() and ((gh >= 0) & (hops < 0)).any()
    state, hops = sc.with_turn(150000).levels(p["start"])
    assert state.max() > 32 and ((gh >= 0) & (hops > gh)).any()
