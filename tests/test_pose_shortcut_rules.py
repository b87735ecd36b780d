"""CPU checks of tests/pose_shortcut_ref.py, the numpy restatement of wa_grid_pose_shortcut (include/weldacs.h, rules 27 - 29): the
identities the header states, the guarantees it lists as consequences, the recorded results of the project's own scenes, and
cover_open against an independent enumeration in exact fractions.  No device here; tests/test_gpu_pose_shortcut.py holds the library
to the restatement byte for byte."""
from fractions import Fraction

import numpy as np
import pytest

import pose_ref as PR
import pose_shortcut_ref as PS
import shortcut_ref as SR
import torch_ref as TR


def scene_of(c, max_turn=None):
    return PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"] if max_turn is None else max_turn, c.get("opened"))


@pytest.fixture(scope="module")
def scenes():
    return PS.scene_paths()


@pytest.fixture(scope="module")
def tunnel():
    c = PR.tunnel_case()
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"])
    _, ids, ks = sc.path(c["points"][0], c["points"][1], c["pins"][0], c["pins"][1])
    return dict(c, ids=ids, ks=ks)


def check_guarantees(sc, ids, ks, w, h, max_span):
    """what rule 28 promises of any result"""
    L = len(ids)
    assert len(w) == len(h) and h[-1] == -1
    assert w[0] == 0 and w[-1] == L - 1 and (np.diff(w) > 0).all() and (np.diff(w) <= max_span).all()
    before = -1
    for t in range(len(w) - 1):
        a, j, hold = int(w[t]), int(w[t + 1]), int(h[t])
        if hold < 0:
            assert j == a + 1, "only the fallback hop is unheld"
            before = -1
            continue
        assert hold in (ks[a], ks[j])
        assert sc.opened[sc.cover(ids[a], ids[j]), hold].all(), "the cover of a held segment is open under its hold"
        # the turns at the two waypoints: k_a -> hold at a, hold -> k_j at j, each between adjacent directions open at that voxel
        assert sc.adj[ks[a], hold] and sc.adj[hold, ks[j]]
        assert sc.opened[ids[a], hold] and sc.opened[ids[j], hold]
        if before >= 0:   # consecutive holds across waypoint a pass through k_a
            assert sc.adj[before, ks[a]] and sc.adj[ks[a], hold]
        before = hold


@pytest.mark.parametrize("max_span", [1, 5, 64, 128])
def test_identity_a_point_tool_is_the_plain_shortcut(tunnel, max_span):
    grid = tunnel["grid"]
    free, _, (nx, ny, _), axes = grid
    sc = PS.Scene(grid, tunnel["dirs"], PS.point_tool(), -1)
    assert np.array_equal(sc.opened, np.repeat((np.asarray(free).ravel() != 0)[:, None], sc.K, 1))
    ids = tunnel["ids"]
    want_w, want_len = SR.shortcut(free, nx, ny, *axes, ids, max_span)
    rs = np.random.RandomState(max_span)
    for ks in (tunnel["ks"], rs.randint(0, sc.K, len(ids)), np.zeros(len(ids), np.int32)):
        w, h, length = sc.shortcut(ids, ks, max_span)
        assert np.array_equal(w, want_w) and length == want_len
    assert max_span == 1 or len(want_w) < len(ids)


def test_identity_b_span_1_keeps_every_node(scenes):
    for name, c in scenes.items():
        w, h, _ = scene_of(c).shortcut(c["ids"], c["ks"], 1)
        assert np.array_equal(w, np.arange(len(c["ids"]))), name


def test_identity_c_no_turn_joins_equal_directions(scenes):
    for name, c in scenes.items():
        sc = scene_of(c, 0)
        assert len({tuple(q) for q in sc.q.tolist()}) == sc.K, "distinct quantised directions"
        w, h, _ = sc.shortcut(c["ids"], c["ks"], 128)
        held = 0
        for t in range(len(w) - 1):
            if h[t] >= 0:
                held += 1
                assert c["ks"][w[t]] == c["ks"][w[t + 1]] == h[t], name
        assert held > 0, name


@pytest.mark.parametrize("max_span", [2, 7, 128])
def test_guarantees_on_the_scenes(scenes, tunnel, max_span):
    for name, c in list(scenes.items()) + [("tunnel", tunnel)]:
        sc = scene_of(c)
        w, h, _ = sc.shortcut(c["ids"], c["ks"], max_span)
        check_guarantees(sc, c["ids"], c["ks"], w, h, max_span)


def test_guarantees_on_paths_that_are_no_pose_paths():
    """random direction indices on a lattice path: adjacency fails, covers close, holds of -1 appear"""
    r = PS.wide_row()
    rs = np.random.RandomState(5)
    sc = PS.Scene(r["grid"], r["dirs"], r["tool"], 30000, r["opened"])
    for _ in range(4):
        ks = rs.randint(0, sc.K, len(r["ids"])).astype(np.int32)
        w, h, _ = sc.shortcut(r["ids"], ks, 16)
        check_guarantees(sc, r["ids"], ks, w, h, 16)
        assert (h[:-1] < 0).any() and (h[:-1] >= 0).any()


def test_recorded_results(scenes):
    c = scenes["pillars6"]
    assert len(c["ids"]) == 12
    ws, hs, _, s = scene_of(c).batch([c["ids"]], [c["ks"]], 128)
    assert ws[0].tolist() == [0, 3, 6, 8, 9, 10, 11] and hs[0].tolist() == [0, 38, 80, 106, 122, 128, -1] and s["n_unheld"] == 0
    c = scenes["pillars4"]
    assert len(c["ids"]) == 14 and (c["ks"].min(), c["ks"].max()) == (0, 129)
    ws, hs, _, s = scene_of(c).batch([c["ids"]], [c["ks"]], 128)
    assert len(ws[0]) - 1 == 9 and s["n_unheld"] == 5 and s["n_held_start"] + s["n_held_end"] == 4
    c = scenes["wide"]
    assert len(c["ids"]) == 45 and len(set(c["ks"].tolist())) == 5
    ws, hs, _, s = scene_of(c).batch([c["ids"]], [c["ks"]], 128)
    assert ws[0].tolist() == [0, 14, 28, 29, 30, 36, 38, 44] and hs[0].tolist() == [0, 0, 2, 7, 23, 23, 15, -1]
    q, holds = scene_of(c).q, hs[0][:-1]
    turn = max(int(TR.turn(q[a], q[b])) for a, b in zip(holds[:-1], holds[1:]))   # every segment is held
    assert s == dict(n_paths=1, n_nodes=45, n_waypoints=8, n_held_start=6, n_held_end=1, n_unheld=0, max_hold_turn=turn) and turn > 0


def test_the_plain_shortcut_cannot_be_held(scenes):
    """why the call exists: what wa_grid_path_shortcut makes of these pose paths has no end direction open along it"""
    for name, n_seg in (("pillars4", 1), ("pillars6", 1), ("wide", 2)):
        c = scenes[name]
        sc = scene_of(c)
        free, _, (nx, ny, _), _ = c["grid"]
        w = SR.waypoints(free, nx, ny, c["ids"], 128)
        assert len(w) - 1 == n_seg, name
        for a, j in zip(w[:-1], w[1:]):
            assert sc.hold(c["ids"][a], c["ks"][a], c["ids"][j], c["ks"][j]) == -1, name


def interval_cover(a, b):
    """the supercover by wa_traj_clearance's header text, in exact fractions: for every voxel of the bounding box, per axis the set of
    t (every t when d_c = 0 and v_c = a_c, none when v_c != a_c, else the closed interval between (2 (v_c - a_c) - 1) / (2 d_c) and
    (2 (v_c - a_c) + 1) / (2 d_c)); the voxel belongs iff [0, 1] and the three sets share a t"""
    d = [b[c] - a[c] for c in range(3)]
    out = set()
    for x in range(min(a[0], b[0]), max(a[0], b[0]) + 1):
        for y in range(min(a[1], b[1]), max(a[1], b[1]) + 1):
            for z in range(min(a[2], b[2]), max(a[2], b[2]) + 1):
                v = (x, y, z)
                lo, hi, ok = Fraction(0), Fraction(1), True
                for c in range(3):
                    if d[c] == 0:
                        ok = ok and v[c] == a[c]
                        continue
                    e = sorted((Fraction(2 * (v[c] - a[c]) - 1, 2 * d[c]), Fraction(2 * (v[c] - a[c]) + 1, 2 * d[c])))
                    lo, hi = max(lo, e[0]), min(hi, e[1])
                if ok and lo <= hi:
                    out.add(v)
    return out


def test_cover_open_against_the_interval_rule(scenes):
    c = scenes["wide"]
    sc = scene_of(c)
    nx, ny, nz = sc.dims
    rs = np.random.RandomState(11)
    pairs = [(int(c["ids"][0]), int(c["ids"][-1])), (0, sc.n - 1), (5, 5)]
    pairs += [(int(a), int(b)) for a, b in rs.randint(0, sc.n, (40, 2))]
    pairs += [(SR._id(3, 1, 1, nx, ny), SR._id(9, 4, 3, nx, ny)), (SR._id(9, 4, 3, nx, ny), SR._id(3, 1, 1, nx, ny))]   # ties of two and three axes
    seen = set()
    for va, vm in pairs:
        cover = interval_cover(SR.voxel(va, nx, ny), SR.voxel(vm, nx, ny))
        assert {SR.voxel(w, nx, ny) for w in sc.cover(va, vm)} == cover
        idx = np.array([(z * ny + y) * nx + x for x, y, z in cover], np.int64)
        for k in rs.randint(0, sc.K, 6):
            want = bool(sc.opened[idx, k].all())
            assert sc.cover_open(va, vm, k) == want
            seen.add(want)
    assert seen == {True, False}
