"""CPU tests of tests/pose_diag_ref.py, the numpy restatement of the diagonal pose paths (include/weldacs.h, rules 43 - 47 of the torch
section): against a heap Dijkstra over explicit states, the five identities of rule 45 (against pose_weighted_ref, pose_ref and
chamfer_weighted_ref), the path conditions, and the table of DESIGN 4z.  tests/test_gpu_pose_diag.py compares the kernels with the
restatement."""
import numpy as np
import pytest

import chamfer_weighted_ref as CW
import pose_diag_ref as PD
import pose_ref as PR
import pose_weighted_ref as PW
import reach_ref as RR
import torch_ref as TR


def dist_pen(grid, near=2, mid=1):
    """a penalty array from the distance field: `near` next to the metal, `mid` within two voxels, 0 elsewhere; 99 on the metal (ignored)"""
    free, d2 = np.asarray(grid[0]).ravel() != 0, np.asarray(grid[1]).ravel()
    return np.where(~free, 99, np.where(d2 <= 1, near, np.where(d2 <= 4, mid, 0))).astype(np.uint8)


@pytest.fixture(scope="module")
def boxes():
    """pose_ref.box_case(0 .. 3) with steps 3-4-5, up to two turn bands and a penalty"""
    out = []
    for seed in range(4):
        c = PR.box_case(seed)
        base = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
        bands = PW.bands_upto(c["dirs"], c["max_turn"], 2)
        tc = [0, 2, 5][:len(bands) + 1]
        pen = dist_pen(c["grid"])
        args = (c["grid"], c["dirs"], c["tool"], c["max_turn"])
        out.append(dict(c=c, base=base, bands=bands, tc=tc, pen=pen, pts=c["points"], args=args,
                        sc=PD.Scene(*args, PD.Costs([3, 4, 5], bands, tc, pen), base)))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_levels_equal_a_heap_dijkstra(boxes, seed):
    b = boxes[seed]
    sc = b["sc"]
    src = b["pts"][1]
    pinned = int(np.flatnonzero(sc.opened[src])[-1])
    for pin in (-1, pinned):
        state, cost = sc.levels(src, pin)
        assert np.array_equal(state, sc.heap_dist(src, pin)), (seed, pin)
        big = np.where(state >= 0, state, 2 ** 31 - 1).min(0)
        assert np.array_equal(cost, np.where((state >= 0).any(0), big, -1))
        assert (state >= 0).sum() > sc.K and cost[src] == 0
    print("box_case", seed, "K", sc.K, "R", sc.R, "deepest level", sc.max_level)
    assert sc.R == max(3 + max(b["tc"]), 4, 5) + sc.P + 1 and sc.P == 2
    assert sc.max_level > 2 * sc.R          # several trips round the ring


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
def test_identity_1_steps_h_2h_3h_are_the_weighted_pose_paths(boxes, h):
    """no pen, any turn costs: a diagonal buys nothing and the faces are asked first"""
    b = boxes[0] if h % 2 else boxes[2]
    pts = b["pts"]
    got = PD.Scene(*b["args"], PD.Costs([h, 2 * h, 3 * h], b["bands"], b["tc"]), b["base"])
    want = PW.Scene(*b["args"], PW.Costs(h, b["bands"], b["tc"]), b["base"])
    for src, pin in ((pts[0], -1), (pts[2], int(np.flatnonzero(got.opened[pts[2]])[0]))):
        gs, gc = got.levels(src, pin)
        ws, wc = want.levels(src, pin)
        assert np.array_equal(gs, ws) and np.array_equal(gc, wc) and (ws > 0).any()
    s, e = [pts[0]] * 3 + [pts[2]], [pts[1], pts[3], pts[5], pts[4]]
    g, w = got.paths(s, e), want.paths(s, e)
    assert np.array_equal(g[0], w[0]) and (w[0] > 0).all()
    for p in range(len(s)):
        assert np.array_equal(g[1][p], w[1][p]) and np.array_equal(g[2][p], w[2][p])


def test_identity_1_unit_steps_without_turn_costs_are_the_pose_paths():
    c = PR.wide_case()
    base = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], PD.Costs([1, 2, 3], [1000, 50000], [0, 0, 0]), base)
    pts, pins = c["points"], c["pins"]
    for i in (0, 1):
        ws, wh = base.levels(pts[i], pins[i])
        state, cost = sc.levels(pts[i], pins[i])
        assert np.array_equal(state, ws) and np.array_equal(cost, wh)
    s, e, ps, pe = [pts[0], pts[1], pts[4]], [pts[1], pts[3], pts[5]], [pins[0], pins[1], -1], [-1, pins[3], pins[5]]
    got, want = sc.paths(s, e, ps, pe), base.paths(s, e, ps, pe)
    assert np.array_equal(got[0], want[0]) and (want[0] > 0).all()
    for p in range(3):
        assert np.array_equal(got[1][p], want[1][p]) and np.array_equal(got[2][p], want[2][p])


@pytest.mark.parametrize("seed", [0, 3])
def test_identity_2_one_direction_is_the_chamfer_on_the_fit_grid(seed):
    grid, dirs, tool = RR.box_scene(seed, 12)
    dirs = dirs[2:3]
    pen = dist_pen(grid, 5, 2)
    step = [3, 4, 5]
    sc = PD.Scene(grid, dirs, tool, 0, PD.Costs(step, [0], [0, 5], pen))
    fit = RR.fit(grid, dirs, tool, min_dirs=1) != 0
    assert fit.sum() < sc.free.sum()
    ff = np.flatnonzero(fit)
    pts = [int(ff[i]) for i in (len(ff) // 2, 3, len(ff) - 5)]
    state, cost = sc.levels(pts[0])
    want = CW.field(fit, step, pen, sc.dims, pts[0])
    assert np.array_equal(cost, want) and np.array_equal(state[0], want) and (want > 0).any()
    wd, _, wp = CW.paths(fit, step, pen, sc.dims, [pts[0]] * 2, pts[1:])
    gd, gi, gk = sc.paths([pts[0]] * 2, pts[1:])
    assert np.array_equal(gd, wd) and (wd > 0).all()
    for p in range(2):
        assert np.array_equal(gi[p], wp[p]) and not gk[p].any()
        assert sum(sc.moves_by_class(gi[p])[1:]) > 0          # the paths do move diagonally


def test_identity_3_no_turn_gives_one_chamfer_field_per_direction():
    c = PR.box_case(0)
    q = TR.quantise_all(c["dirs"])
    assert len({tuple(r) for r in q.tolist()}) == len(q)          # pairwise distinct
    pen = dist_pen(c["grid"])
    step = [3, 4, 5]
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], 0, PD.Costs(step, [], [0], pen))
    src = c["points"][2]
    state, _ = sc.levels(src)
    shut = 0
    for k in range(sc.K):
        if not sc.opened[src, k]:
            assert (state[k] == -1).all()
            shut += 1
            continue
        assert np.array_equal(state[k], CW.field(sc.opened[:, k], step, pen, sc.dims, src)), k
    print("directions shut at the source:", shut, "of", sc.K)
    assert shut < sc.K


def test_identity_4_scaling_every_cost_scales_the_distances_and_keeps_the_paths(boxes):
    b = boxes[0]
    sc = b["sc"]
    twice = PD.Scene(*b["args"], PD.Costs([3, 4, 5], b["bands"], b["tc"], b["pen"]).scaled(3), b["base"])
    assert twice.steps == [9, 12, 15] and twice.R == 3 * (sc.R - 1) + 1
    pts = b["pts"]
    state, cost = sc.levels(pts[0])
    s2, c2 = twice.levels(pts[0])
    assert np.array_equal(s2, np.where(state >= 0, 3 * state, -1)) and np.array_equal(c2, np.where(cost >= 0, 3 * cost, -1))
    one, two = sc.paths([pts[0]] * 3, pts[1:4]), twice.paths([pts[0]] * 3, pts[1:4])
    assert np.array_equal(3 * one[0], two[0]) and (one[0] > 0).all()
    for p in range(3):
        assert np.array_equal(one[1][p], two[1][p]) and np.array_equal(one[2][p], two[2][p])


def test_identity_5_matrix_symmetry(boxes):
    for seed, b in enumerate(boxes):
        sc, pts = b["sc"], b["pts"][:4]
        m = sc.matrix(pts)                                   # with pen, no pins
        adj = m - sc.pen[pts][None, :]
        assert (m >= 0).all() and np.array_equal(adj, adj.T), (seed, m)
        bare = PD.Scene(*b["args"], PD.Costs([3, 4, 5], b["bands"], b["tc"]), b["base"])
        pins = [int(np.flatnonzero(sc.opened[p])[i % 2 * -1]) for i, p in enumerate(pts)]
        for pp in (None, pins):
            m = bare.matrix(pts, pp)                         # without pen, the same pins on both sides
            assert np.array_equal(m, m.T), (seed, pp, m)


def test_every_path_is_a_path_and_costs_what_it_says(boxes):
    diagonal = 0
    for seed, b in enumerate(boxes):
        sc, pts = b["sc"], b["pts"]
        ka = int(np.flatnonzero(sc.opened[pts[0]])[-1])
        kb = int(np.flatnonzero(sc.opened[pts[3]])[0])
        starts, ends = [pts[0], pts[0], pts[1], pts[2]], [pts[3], pts[3], pts[2], pts[0]]
        ps, pe = [ka, -1, -1, -1], [-1, kb, -1, -1]
        D, ids, ks = sc.paths(starts, ends, ps, pe)
        for p in range(4):
            if D[p] < 0:
                assert ids[p] is None
                continue
            sc.check_path(ids[p], ks[p], starts[p], ends[p], ps[p], pe[p], int(D[p]))
            assert D[p] == sc.dist_to(starts[p], ps[p], ends[p], pe[p])
            diagonal += sum(sc.moves_by_class(ids[p])[1:])
        assert (D >= 0).sum() >= 3, (seed, D)
    assert diagonal > 0


def test_check_path_refuses_an_illegal_diagonal():
    """a corner cut past a voxel where the direction is shut, and a diagonal that changes the direction"""
    c = PR.box_case(0)
    sc = PD.Scene(c["grid"], c["dirs"], c["tool"], -1, PD.Costs([3, 4, 5]))
    nx, ny, _ = sc.dims
    found = 0
    for v in np.flatnonzero(sc.opened[:, 0]).tolist():
        x, y, z = sc.coords(v)
        if x + 1 >= nx or y + 1 >= ny:
            continue
        q = v + 1 + nx
        if sc.opened[q, 0] and not (sc.opened[v + 1, 0] and sc.opened[v + nx, 0]):
            with pytest.raises(AssertionError):
                sc.check_path([v, q], [0, 0], v, q, -1, -1, 4)
            found += 1
            break
    assert found == 1
    v = next(v for v in np.flatnonzero(sc.opened[:, :2].all(1)).tolist() if sc.diag_exists(v, (1, 1, 0), 0) and sc.diag_exists(v, (1, 1, 0), 1))
    sc.check_path([v, v + 1 + nx], [1, 1], v, v + 1 + nx, -1, -1, 4)
    with pytest.raises(AssertionError):
        sc.check_path([v, v + 1 + nx], [0, 1], v, v + 1 + nx, -1, -1, 4)


def test_the_table_of_the_design_note():
    """DESIGN 4z's table: steps 3-4-5 without turn costs, from the case's first point, unpinned, to the others, unpinned: 3 x the hops of
    pose_ref.Scene.levels against the distances with diagonal moves.  The right-hand numbers were produced by a Bellman-Ford over
    explicit states that is not part of the repository; this restatement gives the same."""
    rows = [(PR.wide_case(), [249, 204, 225, 99, 213], [221, 194, 203, 93, 205]),
            (PR.box_case(0), [135, 87, 81, 75, 207], [89, 59, 55, 63, 119]),
            (PR.box_case(2), [93, 111, 120, 129, 207], [69, 65, 74, 83, 119])]
    for c, stairs, diag in rows:
        base = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
        sc = PD.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], PD.Costs([3, 4, 5]), base)
        pts = c["points"]
        _, hops = base.levels(pts[0])
        _, cost = sc.levels(pts[0])
        print(sc.K, c["max_turn"], (3 * hops[pts[1:]]).tolist(), cost[pts[1:]].tolist())
        assert (3 * hops[pts[1:]]).tolist() == stairs and cost[pts[1:]].tolist() == diag
    p = PR.pillars(6)
    base = PR.Scene(p["grid"], p["dirs"], p["tool"], 80000)
    sc = PD.Scene(p["grid"], p["dirs"], p["tool"], 80000, PD.Costs([3, 4, 5]), base)
    assert 3 * base.hops_to(p["start"], -1, p["end"], -1) == 33 and sc.dist_to(p["start"], -1, p["end"], -1) == 33


def test_the_narrow_pillars_stay_unreachable():
    p = PR.pillars(4)
    sc = PD.Scene(p["grid"], p["dirs"], p["tool"], 80000, PD.Costs([3, 4, 5]))
    assert sc.dist_to(p["start"], -1, p["end"], -1) == -1
    assert sc.path(p["start"], p["end"])[0] == -1
