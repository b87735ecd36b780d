"""CPU tests of tests/pose_weighted_ref.py, the numpy restatement of the turn-cost pose paths (include/weldacs.h, rules 30 - 36 of the
torch section): against a heap Dijkstra over explicit states, the reductions to pose_ref and to a plain Dijkstra, the matrix identities,
the path conditions, and the table of DESIGN 4w.  tests/test_gpu_pose_weighted.py compares the kernels with the restatement."""
import heapq

import numpy as np
import pytest

import geodesic_ref as GR
import pose_ref as PR
import pose_weighted_ref as PW
import reach_ref as RR

BOX_TURNS = (250000, 60000, -1, 120000)   # max_turn of the 12^3 box scene of each seed


def box12(seed):
    """reach_ref.box_scene(seed, 12): (grid, dirs, tool, max_turn, pen in {0, 2, 5} from d2 <= 1, <= 4, else, bands, four points)"""
    grid, dirs, tool = RR.box_scene(seed, 12)
    free, d2 = np.asarray(grid[0]).ravel() != 0, np.asarray(grid[1]).ravel()
    pen = np.where(d2 <= 1, 0, np.where(d2 <= 4, 2, 5)).astype(np.uint8)
    pen[~free] = 99                                  # an occupied voxel's byte is ignored
    return grid, dirs, tool, BOX_TURNS[seed], pen, PW.bands_upto(dirs, BOX_TURNS[seed], 3), PR.spread_points(grid, 4)


@pytest.fixture(scope="module")
def boxes():
    out = []
    for seed in range(4):
        grid, dirs, tool, max_turn, pen, bands, pts = box12(seed)
        base = PR.Scene(grid, dirs, tool, max_turn)
        tc = [0, 1, 3, 7][:len(bands) + 1]
        out.append(dict(base=base, pen=pen, bands=bands, tc=tc, pts=pts, args=(grid, dirs, tool, max_turn),
                        sc=PW.Scene(grid, dirs, tool, max_turn, PW.Costs(3, bands, tc, pen), base)))
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
    print("box12", seed, "K", sc.K, "R", sc.R, "deepest level", sc.max_level)
    assert sc.max_level > 2 * sc.R          # several trips round the ring
    assert len(sc.weights) == len(b["tc"])  # every class decides something


@pytest.mark.parametrize("costs", [PW.Costs(1), PW.Costs(1, [1000, 50000], [0, 0, 0])], ids=["no_bands", "zero_costs"])
def test_unit_costs_are_the_pose_paths(costs):
    c = PR.wide_case()
    base = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    sc = PW.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], costs, base)
    assert sc.R == 2
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


def test_doubling_every_cost_doubles_the_distances_and_keeps_the_paths(boxes):
    b = boxes[0]
    sc = b["sc"]
    half = PW.Costs(3, b["bands"], b["tc"], b["pen"])
    twice = PW.Scene(*b["args"], half.scaled(2), b["base"])
    assert twice.costs.hop == 6 and twice.R == 2 * (sc.R - 1) + 1
    pts = b["pts"]
    state, cost = sc.levels(pts[0])
    s2, c2 = twice.levels(pts[0])
    assert np.array_equal(s2, np.where(state >= 0, 2 * state, -1)) and np.array_equal(c2, np.where(cost >= 0, 2 * cost, -1))
    one, two = sc.paths([pts[0]] * 3, pts[1:]), twice.paths([pts[0]] * 3, pts[1:])
    assert np.array_equal(2 * one[0], two[0]) and (one[0] > 0).all()
    for p in range(3):
        assert np.array_equal(one[1][p], two[1][p]) and np.array_equal(one[2][p], two[2][p])


def plain_dijkstra(free, entry, dims, src):
    """cheapest totals on the 6-neighbour lattice of free voxels where entering v costs entry[v]"""
    dist = np.full(len(free), -1, np.int64)
    heap = [(0, int(src))]
    while heap:
        d, v = heapq.heappop(heap)
        if dist[v] >= 0:
            continue
        dist[v] = d
        for nb in GR.neighbours(v, dims):
            if free[nb] and dist[nb] < 0:
                heapq.heappush(heap, (d + int(entry[nb]), nb))
    return dist


@pytest.mark.parametrize("seed", [0, 3])
def test_one_direction_is_a_plain_dijkstra_on_the_fit_grid(seed):
    grid, dirs, tool, _, pen, _, _ = box12(seed)
    dirs = dirs[2:3]
    sc = PW.Scene(grid, dirs, tool, 0, PW.Costs(3, [0], [0, 5], pen))
    fit = RR.fit(grid, dirs, tool, min_dirs=1) != 0
    assert fit.sum() < sc.free.sum()
    src = int(np.flatnonzero(fit)[len(np.flatnonzero(fit)) // 2])
    _, cost = sc.levels(src)
    assert np.array_equal(cost, plain_dijkstra(fit, 3 + pen.astype(np.int64), sc.dims, src))


def test_matrix_identities(boxes):
    for seed, b in enumerate(boxes):
        sc, pts = b["sc"], b["pts"]
        m = sc.matrix(pts)                                   # with pen, no pins
        adj = m - sc.pen[pts][None, :]
        assert (m >= 0).all() and np.array_equal(adj, adj.T), (seed, m)
        assert not np.array_equal(m, m.T) or len(set(sc.pen[pts].tolist())) == 1
        bare = PW.Scene(*b["args"], PW.Costs(3, b["bands"], b["tc"]), b["base"])
        pins = [int(np.flatnonzero(sc.opened[p])[i % 2 * -1]) for i, p in enumerate(pts)]
        for pp in (None, pins):
            m = bare.matrix(pts, pp)                         # without pen, the same pins on both sides
            assert np.array_equal(m, m.T), (seed, pp, m)


def test_every_path_is_a_path_and_costs_what_it_says(boxes):
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
        assert (D >= 0).sum() >= 3, (seed, D)


TABLE_COSTS = dict(hop=2, bands=[0, 20000, 80000], turn_costs=[0, 2, 4, 8])


def table_rows():
    """the pairs of DESIGN 4w's table: (name, case dict, max_turn, start, end, end pin)"""
    w = PR.wide_case()
    rows = [("wide", w, 30000, w["points"][4], w["points"][5], 7)]
    for gap in (6, 4):
        p = PR.pillars(gap)
        rows.append(("pillars(%d)" % gap, p, 150000, p["start"], p["end"], -1))
    return rows


def test_the_table_of_the_design_note():
    """(hops, direction changes, sum of U) of pose_paths and of the weighted search"""
    want = {"wide": ((44, 8, 225365), (46, 1, 29092)), "pillars(6)": ((11, 9, 712081), (11, 6, 413860)),
            "pillars(4)": ((13, 8, 605152), (13, 7, 580663))}
    for name, c, max_turn, a, b, pin in table_rows():
        base = PR.Scene(c["grid"], c["dirs"], c["tool"], max_turn)
        sc = PW.Scene(c["grid"], c["dirs"], c["tool"], max_turn, PW.Costs(**TABLE_COSTS), base)
        _, ids, ks = base.path(a, b, -1, pin)
        D, wi, wk = sc.path(a, b, -1, pin)
        got = (PW.path_facts(c["dirs"], ids, ks), PW.path_facts(c["dirs"], wi, wk))
        print(name, got, "cost", D)
        assert got == want[name]
        sc.check_path(wi, wk, a, b, -1, pin, D)


def test_bands_fill_every_class():
    filled = []
    for c in (PR.tunnel_case(), PR.wide_case(), PR.box_case(0), PR.box_case(2)):
        bands = PW.bands_upto(c["dirs"], c["max_turn"], 3)
        cls = PW.turn_class(c["dirs"], bands)
        adj = PR.adjacency(c["dirs"], c["max_turn"])
        assert sorted(set(cls[adj].tolist())) == list(range(len(bands) + 1))
        assert np.array_equal(cls, cls.T) and (np.diag(cls) == 0).all()
        filled.append(len(bands))
    assert filled[0] == 3 and filled[1] == 3, filled
