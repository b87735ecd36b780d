"""GPU tests of the pose family at direction counts across the planes of 64: K = 65, 100 and 128 run k_posew_level<2>, which no other
file launches; K = 193 .. 256 have a fourth plane; K = 128, 192 and 256 fill their last plane (kend == 64 there, bit 63 of the last word
is a live direction, the walk-backs' last lane holds one).  Everything is compared with the numpy restatements (tests/pose_weighted_ref.py,
pose_ref.py, pose_shortcut_ref.py, pose_fit_ref.py) bit for bit.  tests/test_wide_input_rules.py holds the scenes, reads the kernel
selection back from the source and checks that every scene decides something."""
import numpy as np
import pytest

import pose_fit_ref as PF
import pose_shortcut_ref as PS
import test_wide_input_rules as WR
from test_gpu_pose_fit import same as same_fit
from test_gpu_pose_weighted import all_pairs, grid_of, same_paths
from welding_robot_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def costs_of(c):
    return api.pose_costs(WR.PLANES_TABLE["hop"], c["bands"], WR.PLANES_TABLE["turn_costs"], c["pen"])


def field_sources(c):
    """the first voxel with every open direction, and the last point from the last direction of the last plane"""
    return [c["points"][0], c["points"][-1]], [-1, c["pins"][-1]]


@pytest.mark.parametrize("K", WR.PLANE_KS)
def test_weighted_fields_matrix_and_paths(ctx, K):
    c, sc = WR.planes_case(K), WR.planes_scene(K)
    assert sc.K == K and WR.posew_planes(K) == WR.expected_planes()[K]
    g = grid_of(ctx, c["grid"])
    a = (c["dirs"], c["tool"], c["max_turn"], costs_of(c))
    pts, pins = c["points"], c["pins"]
    fp, fpin = field_sources(c)
    cost, state = g.pose_weighted_fields(*a, fp, fpin, states=True)
    assert cost.dtype == state.dtype == np.int32 and state.shape == (2, K, sc.n)
    for i in range(2):
        ws, wc = sc.levels(fp[i], fpin[i])
        assert np.array_equal(cost[i], wc), (K, i, np.flatnonzero(cost[i] != wc)[:5])
        assert np.array_equal(state[i], ws), (K, i, np.argwhere(state[i] != ws)[:5])
    assert np.array_equal(g.pose_weighted_fields(*a, fp, fpin), cost)   # without states
    m = g.pose_weighted_matrix(*a, pts, pins)
    assert np.array_equal(m, sc.matrix(pts, pins)), (K, m)
    assert (m > 0).any() and (np.diag(m) == 0).all()
    m = g.pose_weighted_matrix(*a, pts)
    assert np.array_equal(m, sc.matrix(pts)), (K, m)
    s, e, ps, pe = all_pairs(pts, pins)
    got = g.pose_weighted_paths(*a, s, e, ps, pe)
    same_paths(got, sc.paths(s, e, ps, pe), K)
    planes = set()
    for p in range(len(s)):
        if got[0][p] >= 0:
            sc.check_path(got[1][p], got[2][p], s[p], e[p], ps[p], pe[p], int(got[0][p]))
            planes |= set((got[2][p] >> 6).tolist())
    assert planes == set(range((K + 63) // 64))                          # the walk-backs pass through every plane
    assert np.array_equal(g.occupancy(), np.asarray(c["grid"][0]))
    g.close()
    print("K", K, "planes", WR.posew_planes(K), "R", sc.R, "deepest level", sc.max_level, "points", len(pts))


def few(c):
    """three points: pinned to direction 0, to the last bit of the plane before the last, and to K - 1"""
    idx = [0, len(c["pins"]) - 2, len(c["pins"]) - 1]
    return [c["points"][i] for i in idx], [c["pins"][i] for i in idx]


@pytest.mark.parametrize("K", WR.EXTRA_KS)
def test_pose_calls_with_a_full_last_plane(ctx, K):
    c = WR.planes_case(K)
    sc = c["base"]
    g = grid_of(ctx, c["grid"])
    a = (c["dirs"], c["tool"], c["max_turn"])
    pts, pins = few(c)
    fp, fpin = field_sources(c)
    hops, state = g.pose_fields(*a, fp, fpin, states=True)
    for i in range(2):
        ws, wh = sc.levels(fp[i], fpin[i])
        assert np.array_equal(hops[i], wh) and np.array_equal(state[i], ws), (K, i)
    assert np.array_equal(g.pose_fields(*a, fp, fpin), hops)
    m = g.pose_matrix(*a, pts, pins)
    assert np.array_equal(m, sc.matrix(pts, pins)) and np.array_equal(m, m.T) and (m > 0).any(), (K, m)
    m = g.pose_matrix(*a, pts)
    assert np.array_equal(m, sc.matrix(pts)) and np.array_equal(m, m.T), (K, m)
    s, e, ps, pe = all_pairs(pts, pins)
    got = g.pose_paths(*a, s, e, ps, pe)
    same_paths(got, sc.paths(s, e, ps, pe), K)
    for p in range(len(s)):
        if got[0][p] >= 0:
            sc.check_path(got[1][p], got[2][p], s[p], e[p], ps[p], pe[p], int(got[0][p]))
    g.close()


def planned(K):
    """the restatement's weighted paths between the three points of few(): the pairs with a way, as (ids, ks) lists"""
    c, sc = WR.planes_case(K), WR.planes_scene(K)
    pts, pins = few(c)
    s, e, ps, pe = all_pairs(pts, pins)
    cost, ids, ks = sc.paths(s, e, ps, pe)
    keep = [p for p in range(len(s)) if cost[p] > 0]
    return [ids[p] for p in keep], [ks[p] for p in keep]


@pytest.mark.parametrize("K", WR.EXTRA_KS)
def test_a_shortcut_batch_with_a_full_last_plane(ctx, K):
    c = WR.planes_case(K)
    ids, ks = planned(K)
    assert len(ids) >= 4 and max(int(k.max()) for k in ks) == K - 1
    g = grid_of(ctx, c["grid"])
    wps, wks, holds, lengths, summ = api.pose_shortcut_paths(g, c["dirs"], c["tool"], c["max_turn"], ids, ks, 128)
    ww, wh, wl, ws = PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], c["base"].opened).batch(ids, ks, 128)
    for p in range(len(ids)):
        assert np.array_equal(wps[p], ids[p][ww[p]]) and np.array_equal(wks[p], ks[p][ww[p]]) and np.array_equal(holds[p], wh[p][:-1]), (K, p)
    assert np.array_equal(lengths.view(np.uint64), wl.view(np.uint64)) and summ == ws
    assert summ["n_waypoints"] < summ["n_nodes"] and max(int(h.max()) for h in wh) >= 64 * ((K - 1) // 64)
    g.close()


def fit_case(K):
    """the longest planned path of planned(K), shortened, each leg held by the lowest direction of the last plane that is open along it"""
    c = WR.planes_case(K)
    ids, ks = planned(K)
    p = int(np.argmax([len(i) for i in ids]))
    ps = PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], c["base"].opened)
    w, h, _ = ps.shortcut(ids[p], ks[p], 128)
    way = ids[p][w]
    return c, PF.waypoints(c["grid"], way), WR.last_plane_holds(c, ps, way, h[:-1])


@pytest.mark.parametrize("K", WR.EXTRA_KS)
def test_a_fit_whose_holds_lie_in_the_last_plane(ctx, K):
    c, xyz, holds = fit_case(K)
    lo = 64 * ((K - 1) // 64)
    assert len(holds) >= 2 and (holds >= lo).any()
    r = PF.fit(c["grid"], c["dirs"], c["tool"], xyz, holds, 3, 4.0, 6, 257, c["base"].opened)
    assert (r["seg_dir"] >= lo).any()                                    # segments are held by directions of the last plane
    g = grid_of(ctx, c["grid"])
    same_fit(ctx, g, r, xyz, c["dirs"], c["tool"], holds, 3, 4.0, 6, 257, ("planes", K))
    g.close()
