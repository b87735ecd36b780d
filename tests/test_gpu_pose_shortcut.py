"""GPU tests of wa_grid_pose_shortcut (api.pose_shortcut_paths) against tests/pose_shortcut_ref.py, the header's rules 27 - 29 in numpy:
every output bit-equal, the summary included, and every entry behind a path's waypoints untouched.  tests/test_pose_shortcut_rules.py
checks the restatement itself.

Sizes: k_psc_reach gives one wavefront to an anchor and tests 64 candidates per chunk (a row of 70 nodes at spans 63, 64, 65, 69 and
128: one chunk, a full chunk, a second chunk of one lane, of five); four wavefronts share a workgroup (batches whose node total is
no multiple of 4); a mask word holds 64 directions (K = 130 on the pillars: the two directions of a candidate lie in different planes)."""
import ctypes as C

import numpy as np
import pytest

import pose_ref as PR
import pose_shortcut_ref as PS
import reach_ref as RR
from welding_robot_amd import _lib as L
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG = 1
FILL = -7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def flat(paths, kss):
    paths = [np.ascontiguousarray(p, np.int64).reshape(-1) for p in paths]
    kss = [np.ascontiguousarray(k, np.int32).reshape(-1) for k in kss]
    ids = np.concatenate(paths + [np.zeros(0, np.int64)])
    ks = np.concatenate(kss + [np.zeros(0, np.int32)])
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return ids, ks, off


def raw(g, dirs, tool, max_turn, ids, ks, off, max_span, hold=True, length=True, K=None, dirs_null=False, n_paths=None, summary=True):
    """one raw call on prefilled outputs: (rc, wp, hold, count, length, summary fields as a list)"""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    tool = tool if isinstance(tool, L.ToolBeads) else api.torch_tool(*tool)
    n_paths = len(off) - 1 if n_paths is None else n_paths
    room = (64 if off is None else min(int(off[-1]), 1 << 16)) + 3          # three entries behind the last range
    wp, hd = np.full(room, FILL, np.int64), np.full(room, FILL, np.int32)
    cnt, ln = np.full(max(n_paths, 0) + 1, FILL, np.int32), np.full(max(n_paths, 0) + 1, float(FILL), np.float64)
    s = L.PoseShortcutSummary(*([FILL] * 7))
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    rc = g.ctx.lib.wa_grid_pose_shortcut(g.h, None if dirs_null else p(dirs), len(dirs) if K is None else K, C.byref(tool), max_turn, p(ids), p(ks),
                                         p(off), n_paths, max_span, p(wp), p(hd) if hold else None, p(cnt), p(ln) if length else None,
                                         C.byref(s) if summary else None)
    return rc, wp, hd, cnt, ln, [int(getattr(s, k)) for k, _ in L.PoseShortcutSummary._fields_]


def untouched(out):
    _, wp, hd, cnt, ln, s = out
    return (wp == FILL).all() and (hd == FILL).all() and (cnt == FILL).all() and (ln == FILL).all() and s == [FILL] * 7


def check(g, sc, paths, kss, max_span, what, hold=True, length=True):
    """a raw call against the restatement: waypoints, holds, counts, lengths, summary, and the sentinels behind every range"""
    ids, ks, off = flat(paths, kss)
    ww, wh, wl, ws = sc.batch(paths, kss, max_span)
    out = raw(g, sc.dirs, sc.tool, sc.max_turn, ids, ks, off, max_span, hold, length)
    rc, wp, hd, cnt, ln, s = out
    assert rc == 0, (what, g.ctx.lib.wa_last_error(g.ctx.h))
    n = len(paths)
    assert np.array_equal(cnt[:n], [len(w) for w in ww]) and (cnt[n:] == FILL).all(), (what, cnt)
    if length:
        assert np.array_equal(ln[:n].view(np.uint64), wl.view(np.uint64)) and (ln[n:] == FILL).all(), (what, ln[:n], wl)
    else:
        assert (ln == FILL).all(), what
    for p in range(n):
        a, e = int(off[p]), int(off[p + 1])
        assert np.array_equal(wp[a:a + cnt[p]], ww[p]), (what, p, wp[a:a + cnt[p]], ww[p])
        assert (wp[a + cnt[p]:e] == FILL).all(), (what, p)
        if hold:
            assert np.array_equal(hd[a:a + cnt[p]], wh[p]), (what, p, hd[a:a + cnt[p]], wh[p])
            assert (hd[a + cnt[p]:e] == FILL).all(), (what, p)
    assert (wp[off[-1]:] == FILL).all() and (hd[off[-1]:] == FILL).all(), what
    assert hold or (hd == FILL).all(), what
    assert dict(zip(PS.SUMMARY_FIELDS, s)) == ws, (what, s, ws)
    return out, (ww, wh, wl, ws)


def ps_scene(c, opened=None):
    return PS.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], opened)


# ---- the scenes of the issue: the paths come from Grid.pose_paths
@pytest.mark.parametrize("name", ["pillars4", "pillars6", "wide"])
def test_planned_scenes(ctx, name):
    c = PS.scene_paths()[name]
    g = grid_of(ctx, c["grid"])
    pins = (None, [7]) if name == "wide" else (None, None)
    hops, ids, ks = g.pose_paths(c["dirs"], c["tool"], c["max_turn"], [c["ids"][0]], [c["ids"][-1]], pins[0], pins[1])
    assert np.array_equal(ids[0], c["ids"]) and np.array_equal(ks[0], c["ks"])
    sc = ps_scene(c, c["opened"])
    for span in (1, 3, 128):
        _, (ww, wh, _, ws) = check(g, sc, ids, ks, span, (name, span))
        print(name, span, ww[0].tolist(), wh[0].tolist(), ws)
    if name != "wide":   # K = 130: candidates whose two directions lie in different mask planes are tested and held
        w, h = ww[0], wh[0]
        assert any((ks[0][a] >> 6) != (ks[0][j] >> 6) and hh >= 0 for a, j, hh in zip(w[:-1], w[1:], h[:-1]))
    wps, wks, holds, lengths, summ = api.pose_shortcut_paths(g, c["dirs"], c["tool"], c["max_turn"], ids, ks, 128)
    assert np.array_equal(wps[0], ids[0][ww[0]]) and np.array_equal(wks[0], ks[0][ww[0]]) and np.array_equal(holds[0], wh[0][:-1])
    assert lengths.dtype == np.float64 and summ == ws
    g.close()


def pair_paths(g, c, pts, pins):
    s = [pts[i] for i in range(len(pts)) for j in range(len(pts)) if i != j]
    e = [pts[j] for i in range(len(pts)) for j in range(len(pts)) if i != j]
    ps = [pins[i] for i in range(len(pts)) for j in range(len(pts)) if i != j]
    pe = [pins[j] for i in range(len(pts)) for j in range(len(pts)) if i != j]
    hops, ids, ks = g.pose_paths(c["dirs"], c["tool"], c["max_turn"], s, e, ps, pe)
    keep = [p for p in range(len(s)) if hops[p] >= 0]
    return [ids[p] for p in keep], [ks[p] for p in keep]


@pytest.mark.parametrize("seed", [0, 1])
def test_box_pairs(ctx, seed):
    c = PR.box_case(seed)
    g = grid_of(ctx, c["grid"])
    ids, ks = pair_paths(g, c, c["points"], c["pins"])
    assert len(ids) >= 4
    sc = ps_scene(c)
    for span in (4, 128):
        _, (_, _, _, ws) = check(g, sc, ids, ks, span, ("box", seed, span))
        print("box", seed, span, ws)
    g.close()


def test_tunnel_pairs(ctx):
    c = PR.tunnel_case()
    g = grid_of(ctx, c["grid"])
    ids, ks = pair_paths(g, c, c["points"], c["pins"])
    assert len(ids) == 4 and max(len(p) for p in ids) == 64          # 63 candidates: one lane short of a full chunk
    sc = ps_scene(c)
    _, (_, _, _, ws) = check(g, sc, ids, ks, 128, "tunnel")
    assert ws["n_held_start"] + ws["n_held_end"] > 0
    g.close()


# ---- hand-made paths on the wide scene
@pytest.fixture(scope="module")
def wide(ctx):
    r = PS.wide_row()
    g = grid_of(ctx, r["grid"])
    yield g, r
    g.close()


@pytest.mark.parametrize("span", [63, 64, 65, 69, 128])
def test_row_of_70_across_the_ballot_chunks(wide, span):
    g, r = wide
    sc = PS.Scene(r["grid"], r["dirs"], r["tool"], -1, r["opened"])
    _, (ww, wh, _, _) = check(g, sc, [r["ids"]], [r["ks"]], span, ("row", span))
    assert ww[0].tolist() == ([0, span, 69] if span < 69 else [0, 69]) and (wh[0][:-1] == r["ks"][0]).all()


@pytest.mark.parametrize("span", [64, 128])
def test_row_with_a_direction_that_closes(wide, span):
    g, _ = wide
    r = PS.wide_row(closed=True)
    shut = np.flatnonzero(~r["opened"][r["ids"], r["ks"][0]])
    assert 1 <= len(shut) and 0 < shut[0] and shut[-1] < 69
    sc = PS.Scene(r["grid"], r["dirs"], r["tool"], -1, r["opened"])
    _, (ww, wh, _, ws) = check(g, sc, [r["ids"]], [r["ks"]], span, ("closed row", span))
    assert ws["n_unheld"] == len(shut) + 1 and ww[0].tolist() == [0] + list(range(shut[0] - 1, shut[-1] + 2)) + [69]


def test_diagonal_hops(wide):
    """26-neighbour moves: a free diagonal run, and a step that grazes the edge of the box at x 20 .. 23, y 2 .. 5, z 0 .. 3"""
    g, r = wide
    idx = lambda x, y, z: (z * 9 + y) * 70 + x   # noqa: E731
    run = np.array([idx(2 + t, 1 + min(t, 5), min(t, 4)) for t in range(9)], np.int64)
    graze = np.array([idx(18, 1, 0), idx(19, 2, 0), idx(20, 1, 0), idx(21, 1, 0), idx(22, 0, 1)], np.int64)
    free = np.asarray(r["grid"][0]).ravel()
    assert free[run].all() and free[graze].all() and not free[idx(20, 2, 0)]
    paths = [run, graze, graze[1:3]]
    kss = [PS.lowest_open(r["opened"], p) for p in paths]
    for max_turn in (-1, 30000):
        sc = PS.Scene(r["grid"], r["dirs"], r["tool"], max_turn, r["opened"])
        _, (ww, wh, _, ws) = check(g, sc, paths, kss, 128, ("diagonal", max_turn))
        print("diagonal", max_turn, [w.tolist() for w in ww], [h.tolist() for h in wh], ws)
        assert wh[2].tolist() == [-1, -1]      # the cover of the grazing step holds the occupied (20, 2, 0)


def test_batch_of_short_and_empty_paths(wide):
    g, r = wide
    sc = PS.Scene(r["grid"], r["dirs"], r["tool"], 30000, r["opened"])
    k = int(r["ks"][0])
    rs = np.random.RandomState(3)
    paths = [[], [5], [5, 6], [], [], r["ids"][:9], [69], [68, 69], r["ids"][30:41], []]
    kss = [[], [k], [k, k], [], [], rs.randint(0, sc.K, 9), [0], [k, 0], np.full(11, k), []]
    assert sum(len(p) for p in paths) % 4 != 0
    check(g, sc, paths, kss, 128, "mixed batch")
    check(g, sc, paths[:5], kss[:5], 128, "three nodes")     # fewer nodes than one workgroup's four wavefronts
    out, _ = check(g, sc, [[], []], [[], []], 128, "only empty paths")
    assert out[5] == [2, 0, 0, 0, 0, 0, 0]
    out, _ = check(g, sc, [], [], 128, "no path")
    assert out[5] == [0] * 7


@pytest.mark.parametrize("span", [1, 5, 64, 128])
def test_identity_a_on_the_device(ctx, span):
    """a point tool and no turn limit: the bytes of wa_grid_path_shortcut, whatever the directions"""
    c = PR.tunnel_case()
    g = grid_of(ctx, c["grid"])
    hops, paths = api.geodesic_paths(g, [c["points"][0], c["points"][2]], [c["points"][1], c["points"][3]])
    assert (hops > 30).all()
    rs = np.random.RandomState(span)
    kss = [rs.randint(0, len(c["dirs"]), len(p)).astype(np.int32) for p in paths]
    wps, lengths = api.shortcut_paths(g, paths, span)
    got = api.pose_shortcut_paths(g, c["dirs"], PS.point_tool(), -1, paths, kss, span)
    for p in range(len(paths)):
        assert np.array_equal(got[0][p], wps[p])
        assert np.array_equal(got[2][p], got[1][p][:-1])     # every segment is visible, so it is held with its anchor's direction
    assert np.array_equal(got[3].view(np.uint64), lengths.view(np.uint64))
    assert got[4]["n_unheld"] == 0 and got[4]["n_held_end"] == 0
    g.close()


def test_optional_outputs_may_be_null(wide):
    g, r = wide
    c = PS.scene_paths()["wide"]
    sc = ps_scene(c, c["opened"])
    for hold, length in ((False, True), (True, False), (False, False)):
        check(g, sc, [c["ids"], r["ids"]], [c["ks"], r["ks"]], 128, ("null", hold, length), hold, length)


def test_two_calls_return_the_same_bytes(wide):
    g, r = wide
    c = PS.scene_paths()["wide"]
    ids, ks, off = flat([c["ids"], r["ids"], c["ids"][::-1]], [c["ks"], r["ks"], c["ks"][::-1]])
    a = raw(g, c["dirs"], c["tool"], c["max_turn"], ids, ks, off, 128)
    b = raw(g, c["dirs"], c["tool"], c["max_turn"], ids, ks, off, 128)
    assert a[0] == 0 and b[0] == 0 and a[5] == b[5]
    for x, y in zip(a[1:5], b[1:5]):
        assert x.tobytes() == y.tobytes()


def test_bad_arguments_leave_the_outputs_alone(wide):
    g, r = wide
    c = PS.scene_paths()["wide"]
    dirs, tool, K = c["dirs"], c["tool"], len(c["dirs"])
    ids, ks, off = flat([c["ids"], r["ids"][:5]], [c["ks"], r["ks"][:5]])
    assert raw(g, dirs, tool, 3 * (1 << 20), ids, ks, off, 4096)[0] == 0       # the largest max_turn and span are accepted

    def bad(what, **kw):
        a = dict(dirs=dirs, tool=tool, max_turn=30000, ids=ids, ks=ks, off=off, max_span=128)
        a.update(kw)
        out = raw(g, a.pop("dirs"), a.pop("tool"), a.pop("max_turn"), a.pop("ids"), a.pop("ks"), a.pop("off"), a.pop("max_span"), **a)
        assert out[0] == ARG and untouched(out), what

    bad("max_turn below -1", max_turn=-2)
    bad("max_turn above 3 * 2^20", max_turn=3 * (1 << 20) + 1)
    bad("max_span 0", max_span=0)
    bad("max_span 4097", max_span=4097)
    bad("K = 0", K=0)
    bad("K = 257", K=257)
    bad("NULL dirs", dirs_null=True)
    bad("a direction of zero length", dirs=np.concatenate([dirs[:3], np.zeros((1, 3), np.float32)]))
    bad("a direction that is not finite", dirs=np.concatenate([dirs[:-1], np.full((1, 3), np.nan, np.float32)]))
    no_beads = api.torch_tool(*tool)
    no_beads.n_beads = 0
    bad("a tool without beads", tool=no_beads)
    bad("NULL ids", ids=None)
    bad("NULL ks", ks=None)
    bad("NULL off", off=None, n_paths=2)
    bad("NULL sum", summary=False)
    bad("negative n_paths", n_paths=-1)
    bad("off[0] != 0", off=off + 1)
    bad("decreasing offsets", off=np.array([0, 45, 40], np.int64))
    bad("a path of 2^31 nodes", off=np.array([0, 1 << 31, 1 << 31], np.int64))          # (answered from the offsets: no node is read)
    bad("more than 2^33 nodes", off=np.arange(6, dtype=np.int64) * ((1 << 31) - 1))
    bad("an id below the grid", ids=np.concatenate([ids[:7], [-1], ids[8:]]))
    bad("an id beyond the grid", ids=np.concatenate([ids[:-1], [g.n]]))
    bad("a direction index of K", ks=np.concatenate([ks[:-1], [K]]).astype(np.int32))
    bad("a negative direction index", ks=np.concatenate([[-1], ks[1:]]).astype(np.int32))
    # NULL wp_idx and wp_count: nothing else is written either
    d32 = np.ascontiguousarray(dirs, np.float32)
    t = api.torch_tool(*tool)
    wp, cnt, s = np.full(len(ids), FILL, np.int64), np.full(2, FILL, np.int32), L.PoseShortcutSummary(*([FILL] * 7))
    call = lambda w, n: g.ctx.lib.wa_grid_pose_shortcut(g.h, d32.ctypes.data, K, C.byref(t), 30000, ids.ctypes.data, ks.ctypes.data,   # noqa: E731
                                                        off.ctypes.data, 2, 128, w, None, n, None, C.byref(s))
    assert call(None, cnt.ctypes.data) == ARG and call(wp.ctypes.data, None) == ARG
    assert (wp == FILL).all() and (cnt == FILL).all() and s.n_paths == FILL
    with pytest.raises(api.WeldacsError):
        api.pose_shortcut_paths(g, dirs, tool, 30000, [c["ids"]], [c["ks"] + K], 128)


def test_the_restatement_scene_matches_the_device_masks(wide):
    """open(v, k) of the restatement is what wa_grid_tool_reach returns on the device: the walk reads those very masks"""
    g, r = wide
    mask, _, _ = g.torch_reach(r["dirs"], r["tool"])
    assert np.array_equal(mask, RR.pack(r["opened"]))
