"""The widest inputs the planning calls accept, mirrored from welding_robot_amd/csrc and include/weldacs.h: which k_posew_level a
direction count selects, how many trips the matrix's target lookup takes, how many starts of a seam tour are resident at once, where
the source chunks split.  tests/test_gpu_pose_planes.py, tests/test_gpu_wide_matrices.py and tests/test_gpu_seamtour_wide.py take their
sizes and scenes from this file.  If a constant moves in the source, this test fails, and the GPU cases must be moved with it.

  posew_pick      host_pose_weighted.inc: K <= 64 -> k_posew_level<1>, K <= 128 -> <2>, else <WA_POSE_MAX_W>.  k_posew_level<WMAX> holds
                  the level kernel of both lattices and this is the only pick, so the rule covers the wa_grid_pose_diag_* calls too
  pose_max_w      WA_POSE_MAX_W: planes of 64 directions a state has at most
  max_dirs        WA_TORCH_MAX_DIRS
  pose_stride     pose_lookup_targets: the targets a thread of the source's first block takes lie 256 apart
  geo_stride      geo_lookup_targets: likewise
  max_chunk       WA_GEO_MAX_CHUNK: sources per launch (gridDim.y)
  geo_block       WA_GEO_BLOCK: level launches between two reads of last[] / stop[]
  st_seams        wa_gtsp_seam_tour: 1 .. 1024 seams
  st_starts       ... n_starts and max_passes 1 .. 2^20
  st_per_cu       st_launch: resident workgroups per CU
  st_wave / st_state / st_mpad / st_lds_max   wa_gtsp_seam_tour: who holds a descent and what its LDS holds
  st_block        WA_ST_BLOCK"""
import os
import re

import numpy as np
import pytest

import geodesic_ref as G
import pose_ref as PR
import pose_weighted_ref as PW
import reach_ref as RR
import seamtour_ref as R
import torch_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "welding_robot_amd", "csrc")
SRC = {k: os.path.join(CSRC, f) for k, f in (("posew", "host_pose_weighted.inc"), ("pose", "pose_kernels.hpp"), ("geo", "geodesic_kernels.hpp"),
                                               ("hgeo", "host_geodesic.inc"), ("hst", "host_seamtour.inc"), ("st", "seamtour_kernels.hpp"))}
SRC["h"] = os.path.join(ROOT, "include", "weldacs.h")

# ------------------------------------------------------------------ the table
# rule -> (source, regex over whitespace-collapsed text, its constants in order of appearance)
_LOOKUP = (r"__device__ __forceinline__ void %s_lookup_targets\([^{}]*\) \{ int missing = 0; "
           r"for \(int32_t t = \(int32_t\)threadIdx\.x; t < n_tgt; t \+= (\d+)\) \{")
TABLE = {
    "posew_pick": ("posew", r"const auto kernel = K <= (\d+) \? k_posew_level<(\d+)> : K <= (\d+) \? k_posew_level<(\d+)> : k_posew_level<WA_POSE_MAX_W>;",
                   (64, 1, 128, 2)),
    "pose_max_w": ("pose", r"#define WA_POSE_MAX_W (\d+) ", (4,)),
    "max_dirs": ("h", r"#define WA_TORCH_MAX_DIRS (\d+) ", (256,)),
    "pose_stride": ("pose", _LOOKUP % "pose", (256,)),
    "geo_stride": ("geo", _LOOKUP % "geo", (256,)),
    "max_chunk": ("hgeo", r"static const int32_t WA_GEO_MAX_CHUNK = (\d+);", (65535,)),
    "geo_block": ("hgeo", r"static const int32_t WA_GEO_BLOCK = (\d+);", (32,)),
    "st_seams": ("hst", r"if \(m < 1 \|\| m > (\d+)\) return fail\(ctx, WA_ERR_ARG, \"wa_gtsp_seam_tour: 1 \.\. 1024 seams\"\);", (1024,)),
    "st_starts": ("hst", r"prm->n_starts < 1 \|\| prm->n_starts > \((\d+) << (\d+)\) \|\| prm->max_passes < 1 \|\| prm->max_passes > \((\d+) << (\d+)\)\)",
                  (1, 20, 1, 20)),
    "st_per_cu": ("hst", r"const long long per_cu = std::min<long long>\((\d+) / \(WA_ST_BLOCK / (\d+)\), std::max<long long>\((\d+), "
                         r"\(long long\)\((\d+) \* (\d+) / lds\)\)\);", (32, 64, 1, 160, 1024)),
    "st_wave": ("hst", r"const bool wave = M <= (\d+);", (64,)),
    "st_mpad": ("hst", r"const int Mpad = \(M \+ (\d+)\) & ~(\d+);", (7, 7)),
    "st_state": ("hst", r"const size_t state = \(size_t\)\(wave \? (\d+) : (\d+)\) \* (\d+) \* Mpad \* sizeof\(uint16_t\) \+ \(WA_ST_BLOCK / (\d+)\) \* (\d+);",
                 (4, 1, 2, 64, 16)),
    "st_lds_max": ("hst", r"const size_t lds_max = (\d+) \* (\d+);", (160, 1024)),
    "st_block": ("st", r"#define WA_ST_BLOCK (\d+) ", (256,)),
}
# rules without a constant of their own, stated as they are or the helpers below are wrong
RULES = (
    ("hst", r"const int teams = WA_ST_BLOCK / TEAM; const long long want = \(\(long long\)a\.n_starts \+ teams - 1\) / teams;"),
    ("hst", r"const long long cap = \(long long\)std::max\(1, ctx->prop\.multiProcessorCount\) \* per_cu;"),
    ("hst", r"k_seam_descend<WT, W_LDS, TEAM><<<\(unsigned\)std::min\(want, cap\), WA_ST_BLOCK, lds, ctx->stream>>>\(a\);"),
    ("hst", r"const size_t w_narrow = \(\(size_t\)N2 \* N2 \* 4 \+ 15\) & ~\(size_t\)15, w_wide = \(\(size_t\)N2 \* N2 \* 8 \+ 15\) & ~\(size_t\)15;"),
    ("hst", r"const bool w_lds = wave \|\| \(narrow && w_narrow \+ state <= lds_max\); "
            r"const size_t lds = state \+ \(w_lds \? \(narrow \? w_narrow : w_wide\) : 0\);"),
    ("hst", r"if \(wave\) e = narrow \? st_launch<uint32_t, true, 64>\(ctx, a, lds\) : st_launch<long long, true, 64>\(ctx, a, lds\); "
            r"else if \(w_lds\) e = st_launch<uint32_t, true, 256>\(ctx, a, lds\); "
            r"else e = narrow \? st_launch<uint32_t, false, 256>\(ctx, a, lds\) : st_launch<long long, false, 256>\(ctx, a, lds\);"),
    ("hst", r"if \(w >> 32\) \*narrow = false;"),
    ("st", r"for \(int start = blockIdx\.x \* TEAMS \+ team; start < A\.n_starts; start \+= gridDim\.x \* TEAMS\) \{"),
    ("hgeo", r"cap = std::max<int64_t>\(1, std::min<int64_t>\(cap, std::min<int64_t>\(n_src, WA_GEO_MAX_CHUNK\)\)\);"),
    ("hgeo", r"for \(int32_t s0 = 0; rc == WA_OK && s0 < n_src; s0 \+= c\.cap\) \{ const int32_t ns = std::min\(c\.cap, n_src - s0\);"),
    ("pose", r"if \(tgt && blockIdx\.x == 0\) pose_lookup_targets\("),
    ("geo", r"if \(!__syncthreads_or\(missing\) && threadIdx\.x == 0\) \*stop_s = 1;"),
    ("pose", r"if \(!__syncthreads_or\(missing\) && threadIdx\.x == 0\) \*stop_s = 1;"),
)


def _c(name):
    return TABLE[name][2]


# ------------------------------------------------------------------ what the table says
def posew_planes(K):
    """the WMAX of the k_posew_level a call with K directions launches"""
    k1, w1, k2, w2 = _c("posew_pick")
    assert 1 <= K <= _c("max_dirs")[0]
    return w1 if K <= k1 else w2 if K <= k2 else _c("pose_max_w")[0]


def lookup_trips(n_tgt, thread=0):
    """trips of the target loop that thread `thread` of the source's first block makes"""
    stride = _c("pose_stride")[0]
    assert stride == _c("geo_stride")[0]
    return len(range(thread, n_tgt, stride))


def seam_storage(M, narrow):
    """(TEAM, W in LDS, dynamic LDS bytes) of a tour on M positions, as wa_gtsp_seam_tour computes them"""
    a, b = _c("st_mpad")
    Mpad = (M + a) & ~b
    wave = M <= _c("st_wave")[0]
    s = _c("st_state")
    block = _c("st_block")[0]
    state = (s[0] if wave else s[1]) * s[2] * Mpad * 2 + (block // s[3]) * s[4]
    N2 = 2 * M
    w_narrow, w_wide = (N2 * N2 * 4 + 15) & ~15, (N2 * N2 * 8 + 15) & ~15
    lds_max = _c("st_lds_max")[0] * _c("st_lds_max")[1]
    w_lds = wave or (narrow and w_narrow + state <= lds_max)
    lds = state + ((w_narrow if narrow else w_wide) if w_lds else 0)
    return (_c("st_wave")[0] if wave else block), w_lds, lds


def resident_starts(M, narrow, cus):
    """starts that descend at once on a device of `cus` compute units once n_starts exceeds them: a team's next start is this many on"""
    team, _, lds = seam_storage(M, narrow)
    p = _c("st_per_cu")
    block = _c("st_block")[0]
    per_cu = min(p[0] // (block // p[1]), max(p[2], (p[3] * p[4]) // lds))
    return max(1, cus) * per_cu * (block // team)


MAX_SEAMS = _c("st_seams")[0]
MAX_STARTS = _c("st_starts")[0] << _c("st_starts")[1]
MAX_CHUNK = _c("max_chunk")[0]


# ------------------------------------------------------------------ the source, read back
def _text(src):
    return {k: re.sub(r"\s+", " ", v) for k, v in src.items()}


def mirrored(text):
    """rule -> its constants as the (whitespace-collapsed) sources state them (None: the statement is not there, or not once)"""
    out = {}
    for name, (where, pat, _) in TABLE.items():
        found = set(re.findall(pat, text[where]))
        f = found.pop() if len(found) == 1 else None
        out[name] = None if f is None else tuple(int(x) for x in (f if isinstance(f, tuple) else (f,)))
    for where, pat in RULES:
        out[pat] = bool(re.search(pat, text[where]))
    return out


def _sources():
    out = {}
    for k, p in SRC.items():
        with open(p) as f:
            out[k] = f.read()
    return out


def _want():
    w = {name: c for name, (_, _, c) in TABLE.items()}
    w.update({pat: True for _, pat in RULES})
    return w


def test_the_table_is_what_the_source_states():
    got, want = mirrored(_text(_sources())), _want()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_moving_any_constant_of_a_rule_is_noticed(name):
    """each constant of the rule, changed by one in a copy of the source text, makes the mirror differ -- in that rule"""
    text = _text(_sources())
    where, pat, consts = TABLE[name]
    m = re.search(pat, text[where])
    assert m is not None
    for k in range(1, len(consts) + 1):
        mutated = dict(text, **{where: text[where][:m.start(k)] + str(int(m.group(k)) + 1) + text[where][m.end(k):]})
        got = mirrored(mutated)
        assert got[name] != consts, (name, k)
        assert all(got[o] == w for o, w in _want().items() if o != name), (name, k)


@pytest.mark.parametrize("name,old,new", [
    ("posew_pick", "K <= 64 ? k_posew_level<1>", "K < 64 ? k_posew_level<1>"),
    ("posew_pick", "K <= 128 ? k_posew_level<2>", "K < 128 ? k_posew_level<2>"),
    ("st_wave", "wave = M <= 64;", "wave = M < 64;"),
    ("st_seams", "m > 1024) return fail(ctx, WA_ERR_ARG, \"wa_gtsp_seam_tour: 1", "m >= 1024) return fail(ctx, WA_ERR_ARG, \"wa_gtsp_seam_tour: 1"),
])
def test_changing_a_comparison_is_noticed(name, old, new):
    text = _text(_sources())
    where = TABLE[name][0]
    assert text[where].count(old) == 1, old
    assert mirrored(dict(text, **{where: text[where].replace(old, new)}))[name] is None


def test_the_limits_hang_together():
    assert _c("pose_max_w")[0] * 64 == _c("max_dirs")[0] == 256
    assert MAX_SEAMS == 1024 and MAX_STARTS == 1 << 20 and MAX_CHUNK == 65535
    assert _c("pose_stride")[0] == _c("geo_stride")[0] == 256          # (the level kernels' workgroup: one target per thread and trip)
    assert 2 * (MAX_SEAMS + 1) < 1 << 16                                # (endpoints are uint16)
    assert 7 * (MAX_SEAMS + 1) ** 2 < 1 << 31                           # (move numbers are int)


# ------------------------------------------------------------------ 1. direction counts across the planes
PLANE_KS = (65, 100, 128, 129, 192, 193, 255, 256)
FULL_PLANE_KS = (128, 192, 256)          # kend == 64 in the last plane; run on the wide scene (a tail of 6 lanes, two chunks per row)
EXTRA_KS = (128, 256)                    # also the pose calls, a shortcut batch and a fit
PLANES_TURN = 60000
PLANES_TABLE = dict(hop=2, turn_costs=[0, 1, 3, 6])


def expected_planes():
    return {65: 2, 100: 2, 128: 2, 129: 4, 192: 4, 193: 4, 255: 4, 256: 4}


def near_pen(grid, top=3):
    """a penalty array from the distance field: `top` next to the metal, 1 within two voxels, 0 elsewhere; 200 on the metal (ignored)"""
    free, d2 = np.asarray(grid[0]).ravel() != 0, np.asarray(grid[1]).ravel()
    return np.where(~free, 200, np.where(d2 <= 1, top, np.where(d2 <= 4, 1, 0))).astype(np.uint8)


def plane_pins(K):
    """0, 63, 64, K - 1 and the last bit of every plane"""
    return sorted({0, 63, 64, K - 1} | {min(64 * w + 63, K - 1) for w in range((K + 63) // 64)})


_PLANES = {}


def planes_case(K):
    """the scene of one direction count: pose_ref.wide_scene()'s grid and tool where the last plane is full, reach_ref.box_scene(1, 12)'s
    elsewhere; K directions on a cap of half angle 2.2, PLANES_TURN, three bands at quantiles of the adjacent turns, near_pen.  Three
    voxels with every direction open carry the points: `points` / `pins` name them in turn with plane_pins(K), so the pinned matrix
    starts and ends in every plane.  Computed once per process, never modified.
    dict(grid, dirs, tool, max_turn, bands, pen, points, pins, voxels, base)"""
    if K not in _PLANES:
        if K in FULL_PLANE_KS:
            w = PR.wide_scene()
            grid, tool = w["grid"], w["tool"]
        else:
            grid, _, tool = RR.box_scene(1, 12)
        dirs = T.fib_dirs(K, 2.2, (0.3, -0.2, 1.0))
        base = PR.Scene(grid, dirs, tool, PLANES_TURN)
        wide_open = np.flatnonzero(base.opened.all(1))
        vox = [int(wide_open[i]) for i in np.linspace(0, len(wide_open) - 1, 3).astype(np.int64)]
        pins = plane_pins(K)
        _PLANES[K] = dict(grid=grid, dirs=dirs, tool=tool, max_turn=PLANES_TURN, bands=PW.bands_for(dirs, PLANES_TURN, 3), pen=near_pen(grid),
                          points=[vox[i % 3] for i in range(len(pins))], pins=pins, voxels=vox, base=base)
    return _PLANES[K]


def planes_scene(K):
    """pose_weighted_ref.Scene of planes_case(K), shared by the CPU and the GPU tests (its fields are kept)"""
    c = planes_case(K)
    if "scene" not in c:
        c["scene"] = PW.Scene(c["grid"], c["dirs"], c["tool"], c["max_turn"], PW.Costs(PLANES_TABLE["hop"], c["bands"], PLANES_TABLE["turn_costs"], c["pen"]),
                              c["base"])
    return c["scene"]


def last_plane_holds(c, sc, ids, holds):
    """per leg of a shortened path (waypoint ids, holds) a direction of the last plane: on the even legs the highest that is open along
    the leg's whole cover, on the odd legs the highest that is open at both of its ends (the curve between them may find it closed);
    the planned hold where there is none"""
    K = sc.K
    lo = 64 * ((K - 1) // 64)
    out = []
    for i, (a, b, h) in enumerate(zip(ids[:-1], ids[1:], holds)):
        at = sc.cover(a, b) if i % 2 == 0 else np.array([a, b], np.int64)
        ok = np.flatnonzero(sc.opened[at, lo:].all(0))
        out.append(lo + int(ok[-1]) if len(ok) else int(h))
    return np.array(out, np.int32)


@pytest.mark.parametrize("K", PLANE_KS)
def test_every_direction_count_selects_its_kernel_and_its_scene_decides(K):
    assert posew_planes(K) == expected_planes()[K]
    assert (K in FULL_PLANE_KS) == (K % 64 == 0)
    c = planes_case(K)
    base = c["base"]
    W = (K + 63) // 64
    free = base.free
    assert (free[:, None] & ~base.opened).any() and base.opened.any()                      # some directions are blocked, not all
    mask = RR.pack(base.opened)
    assert mask.shape[0] == W and all(mask[w].any() for w in range(W))                     # every plane of the open masks is in use
    assert (mask[W - 1] >> np.uint64((K - 1) & 63)).any()                                   # ... up to its last live bit
    assert 0 < base.adj.mean() < 1 and not base.adj.all(1).any()                            # the adjacency is neither empty nor full
    off = base.adj & ~np.eye(K, dtype=bool)
    assert all(off[:, 64 * w:64 * w + 64].any() and off[64 * w:64 * w + 64].any() for w in range(W))
    assert len(c["bands"]) == 3 and len(set(c["pen"][free].tolist())) == 3
    assert sorted(set(c["pins"])) == c["pins"] and {0, 63, 64, K - 1} <= set(c["pins"]) and {p >> 6 for p in c["pins"]} == set(range(W))
    assert len(set(c["voxels"])) == 3 and base.opened[c["voxels"]].all()
    sc = planes_scene(K)
    assert len(sc.weights) == 4 and sc.P == 3 and sc.R == 12
    state, cost = sc.levels(c["points"][-1], c["pins"][-1])                                # from the last direction of the last plane
    assert state[K - 1, c["points"][-1]] == 0 and (state[:, c["points"][-1]] == 0).sum() == 1
    reached = (state >= 0)
    assert all(reached[64 * w:64 * w + 64].any() for w in range(W)) and reached[K - 1].sum() > 1
    assert (cost[free] > 0).any() and (cost[free] < 0).any()                               # free voxels without an open direction stay at -1
    m = sc.matrix(c["points"][-3:], c["pins"][-3:])
    assert (m > 0).any()


# ------------------------------------------------------------------ 2. matrices with more than 256 points
MATRIX_DIMS = (12, 12, 12)
MATRIX_SIZES = (257, 300, 513)           # the issue's lists: a second trip of one lane, of 44 lanes, a third trip of one lane
OPEN_SIZE = 258                          # and one list without a pocket point: its rows complete, stop[s] is set
MATRIX_K = 5
MATRIX_TURN = 300000


def matrix_free():
    """12^3 with two boxes and a shell of metal (x, y, z 4 .. 8) around a sealed pocket of 3^3 free voxels (5 .. 7)"""
    f = np.ones((12, 12, 12), np.uint8)
    f[4:9, 4:9, 4:9] = 0
    f[5:8, 5:8, 5:8] = 1
    f[0:3, 8:12, 9:11] = 0
    f[9:12, 0:4, 2:4] = 0
    return f.reshape(-1)


def pocket_ids():
    z, y, x = np.meshgrid(np.arange(5, 8), np.arange(5, 8), np.arange(5, 8), indexing="ij")
    return ((z * 12 + y) * 12 + x).ravel()


_MATRIX = {}


def matrix_case():
    """dict(free, grid, dims, dirs, tool, lists): lists[P] = (points int64 [P], pins int32 [P]).  The issue's three lists are prefixes of
    one seeded list; voxel `dup` stands at 3, 100, 256, 299 and 512 (the first target of thread 0's second and third trip) with a
    different pin each time, pocket voxels at 7, 200, 257, 258, 400 and 511.  lists[OPEN_SIZE] has no pocket point and only voxels with every direction open (`dup` at 3, 100
    and 256 again): every row of all six calls completes."""
    if not _MATRIX:
        free = matrix_free()
        rs = np.random.RandomState(2024)
        pocket = pocket_ids()
        outside = np.setdiff1d(np.flatnonzero(free), pocket)
        pts = outside[rs.randint(len(outside), size=513)].astype(np.int64)
        pins = rs.randint(-1, MATRIX_K, size=513).astype(np.int32)
        dup = int(outside[len(outside) // 3])
        for k, at in enumerate((3, 100, 256, 299, 512)):
            pts[at], pins[at] = dup, k - 1
        for k, at in enumerate((7, 200, 257, 258, 400, 511)):
            pts[at] = pocket[(5 * k + 13) % 27]
        pts[258] = pts[257]                                                                 # (two points on one pocket voxel)
        pins[257], pins[258] = -1, 0
        lists = {P: (pts[:P].copy(), pins[:P].copy()) for P in MATRIX_SIZES}
        grid = T.make_grid(free, MATRIX_DIMS)
        dirs, tool = T.fib_dirs(MATRIX_K, 1.2, (0.3, -0.2, 1.0)), T.rod(3, 40, 0)
        opened = RR.open_dirs(grid, dirs, tool)
        wide_open = np.intersect1d(outside, np.flatnonzero(opened.all(1)))
        open_pts = wide_open[rs.randint(len(wide_open), size=OPEN_SIZE)].astype(np.int64)
        open_pts[[3, 100, 256]] = wide_open[len(wide_open) // 3]
        lists[OPEN_SIZE] = (open_pts, pins[:OPEN_SIZE].copy())
        _MATRIX.update(free=free, grid=grid, dims=MATRIX_DIMS, dirs=dirs, tool=tool, lists=lists, dup=dup, opened=opened)
    return _MATRIX


def test_the_point_lists_reach_the_later_trips_and_leave_rows_open():
    c = matrix_case()
    free, pocket = c["free"], set(pocket_ids().tolist())
    assert [lookup_trips(P) for P in MATRIX_SIZES + (OPEN_SIZE,)] == [2, 2, 3, 2]
    assert [lookup_trips(P, 255) for P in MATRIX_SIZES] == [1, 1, 2] and lookup_trips(300, 43) == 2 and lookup_trips(300, 44) == 1
    f0 = G.field(free, MATRIX_DIMS, 0)
    inside = G.field(free, MATRIX_DIMS, int(pocket_ids()[0]))
    assert set(np.flatnonzero(inside >= 0).tolist()) == pocket and not (f0[list(pocket)] >= 0).any()      # sealed
    assert (f0[free != 0] >= 0).sum() == free.sum() - 27
    for P in MATRIX_SIZES:
        pts, pins = c["lists"][P]
        assert len(pts) == P and free[pts].all()
        in_pocket = np.array([int(p) in pocket for p in pts])
        assert in_pocket[:256].any() and (P == 257 or in_pocket[256:].any()) and not in_pocket.all()
        at = np.flatnonzero(pts == c["dup"])
        assert len(at) >= 3 and at[0] < 256 <= at[-1] and len(set(pins[at].tolist())) >= 3
        m = G.matrix(free, MATRIX_DIMS, pts[:40])
        assert (m == -1).any() and (m > 0).any()
    pts, _ = c["lists"][OPEN_SIZE]
    assert not any(int(p) in pocket for p in pts) and (G.matrix(free, MATRIX_DIMS, pts[:40]) >= 0).all()
    # the pose calls: directions are blocked beside the metal, some are open inside the pocket, the turn limit cuts the adjacency
    sc = PR.Scene(c["grid"], c["dirs"], c["tool"], MATRIX_TURN, c["opened"])
    assert sc.opened[pts].all() and len(set(pts.tolist())) > 100
    f = free != 0
    assert (f[:, None] & ~sc.opened).any() and sc.opened[pocket_ids()].any() and 0 < sc.adj.mean() < 1
    pts, pins = c["lists"][513]
    a, b = np.flatnonzero(pts == c["dup"])[:2]
    state, hops = sc.levels(pts[a], pins[a])
    other, _ = sc.levels(pts[b], pins[b])
    assert not np.array_equal(state, other)                                                  # the pins of two duplicates give two rows


# ------------------------------------------------------------------ 3. seam tours wide and large
def euclid(m, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    p = (rs.uniform(0, 10, (2 * m, 3)) * scale).astype(np.float64)
    d = np.zeros((2 * m, 2 * m))
    for c in range(3):
        d += (p[:, None, c] - p[None, :, c]) ** 2
    return np.sqrt(d)


def given_start(m, seed):
    rs = np.random.RandomState(seed)
    return rs.permutation(m).astype(np.int32), rs.randint(0, 2, m).astype(np.uint8)


# name -> (m, closed, scale, max_passes, (TEAM, W in LDS, narrow)): one job per storage case, n_starts = 2 * resident + 3
MULTI = {
    "wave_narrow": (5, True, 1.0, 1 << 20, (64, True, True)),
    "wave_wide": (40, True, 1e4, 1 << 20, (64, True, False)),
    "group_lds": (70, True, 1.0, 1 << 20, (256, True, True)),
    "group_global": (120, True, 1.0, 3, (256, False, True)),
}
# name -> (m, closed, scale): n_starts 2, a given start, max_passes 3
LARGE = {
    "1024_closed": (1024, True, 1.0),
    "1024_open": (1024, False, 1.0),
    "513": (513, True, 1.0),
    "300_open": (300, False, 1.0),
    "1024_open_wide": (1024, False, 1e4),
}


def multi_job(name):
    m, closed, scale, max_passes, _ = MULTI[name]
    return euclid(m, 500 + m, scale), dict(closed=closed, or_len=3, max_passes=max_passes, seed=0xBEEF + m)


def large_job(name):
    m, closed, scale = LARGE[name]
    o0, d0 = given_start(m, m)
    return euclid(m, 700 + m + (0 if closed else 1), scale), dict(closed=closed, or_len=3, n_starts=2, max_passes=3, seed=0xFACE + m, order0=o0, dir0=d0)


def multi_starts(name, cus):
    m, closed, scale, _, (_, _, narrow) = MULTI[name]
    return 2 * resident_starts(m if closed else m + 1, narrow, cus) + 3


def sampled_starts(n_starts, resident, seed=5):
    """start 0, 1, the last, the first and last of the second trip, the first two of the third, and 200 seeded picks without repetition
    (every start where there are no more than 400)"""
    assert n_starts == 2 * resident + 3
    rs = np.random.RandomState(seed)
    fixed = [0, 1, n_starts - 1, resident, 2 * resident - 1, 2 * resident, 2 * resident + 1]
    picks = range(n_starts) if n_starts <= 400 else rs.choice(n_starts, 200, replace=False).tolist()
    return sorted(set(fixed) | set(picks))


def descents(job):
    """worker: (name, starts) -> [(start, final cost, passes, capped)] of those starts of MULTI[name], each from its own descent
    (seamtour_ref.random_start + descend: a start does not depend on the others)"""
    name, starts = job
    m, closed, _, max_passes, _ = MULTI[name]
    d, kw = multi_job(name)
    W = R.quantise(d, m, closed)
    M = m if closed else m + 1
    out = []
    for r in starts:
        E, p, c = R.descend(R.start0(m, closed) if r == 0 else R.random_start(M, kw["seed"], r), W, kw["or_len"], max_passes)
        out.append((int(r), R.tour_cost(E, W), p, c))
    return out


def test_resident_starts_in_the_three_storage_cases():
    # (TEAM, W in LDS, LDS bytes) by hand: M = 5: W 10 x 10 x 4 = 400, state 4 x 2 x 8 x 2 + 64 = 192; M = 40 wide: 80 x 80 x 8 = 51 200,
    # state 4 x 2 x 40 x 2 + 64 = 704; M = 70: 140 x 140 x 4 = 78 400, state 2 x 72 x 2 + 64 = 352; M = 120: 240 x 240 x 4 > 160 KiB
    assert seam_storage(5, True) == (64, True, 592)
    assert seam_storage(40, False) == (64, True, 51904)
    assert seam_storage(70, True) == (256, True, 78752)
    assert seam_storage(120, True) == (256, False, 544)
    assert seam_storage(101, True)[1] and not seam_storage(102, True)[1] and not seam_storage(70, False)[1]
    # 256 compute units: 8 workgroups of 4 teams; 160 KiB / 51 904 = 3 workgroups of 4; 2 workgroups of 1; 8 of 1
    assert [resident_starts(M, nw, 256) for M, nw in ((5, True), (40, False), (70, True), (120, True))] == [8192, 3072, 512, 2048]
    assert resident_starts(5, True, 1) == 32 and resident_starts(5, True, 0) == 32 and resident_starts(1025, False, 304) == 304 * 8
    for name, (m, closed, scale, _, want) in MULTI.items():
        M = m if closed else m + 1
        W = R.quantise(multi_job(name)[0], m, closed)
        narrow = not (W >> 32).any()
        assert (seam_storage(M, narrow)[:2] + (narrow,)) == want, name
        for cus in (1, 64, 256, 304):
            n = multi_starts(name, cus)
            res = resident_starts(M, narrow, cus)
            assert 2 * res < n <= MAX_STARTS and -(-n // (256 // want[0])) > res // (256 // want[0])       # the grid is capped; three trips
            s = sampled_starts(n, res)
            assert len(s) >= min(200, n) and {0, 1, n - 1, res, 2 * res - 1, 2 * res} <= set(s)


@pytest.mark.parametrize("name", sorted(MULTI))
def test_the_multi_start_descents_move(name):
    m, closed, _, max_passes, _ = MULTI[name]
    d, kw = multi_job(name)
    W = R.quantise(d, m, closed)
    M = m if closed else m + 1
    moved = 0
    for r in (1, 2, 3, 1000, 5000):
        E0 = R.random_start(M, kw["seed"], r)
        E, passes, capped = R.descend(E0, W, 3, max_passes)
        moved += E != E0
        assert R.tour_cost(E, W) <= R.tour_cost(E0, W)
        if max_passes == 3:
            assert capped == 1 and passes == 3                                               # the cap binds: n_capped counts
    assert moved >= (3 if m == 5 else 5)


@pytest.mark.parametrize("name", sorted(LARGE))
def test_the_large_jobs_are_at_the_limits_and_their_descents_move(name):
    m, closed, scale = LARGE[name]
    M = m if closed else m + 1
    assert M > 201 and m <= MAX_SEAMS
    d, kw = large_job(name)
    W = R.quantise(d, m, closed)
    assert bool((W >> 32).any()) == (scale > 1)                                              # a 64-bit W exactly where the costs are scaled
    assert seam_storage(M, scale == 1)[:2] == (256, False)
    for E in (R.start0(m, closed, kw["order0"], kw["dir0"]), R.random_start(M, kw["seed"], 1)):
        delta, num = R.best_move(E, W, 3)
        assert delta < 0 and 0 <= num < 7 * M * M


def test_the_large_jobs_cover_the_issue():
    Ms = sorted((m if c else m + 1) for m, c, _ in LARGE.values())
    assert Ms == [301, 513, 1024, 1025, 1025] and 202 <= Ms[0] <= 512
    assert 7 * 1025 ** 2 > 7_300_000 and (2 * 1025) ** 2 * 8 > 33_000_000                    # move numbers and the bytes of the wide W


# ------------------------------------------------------------------ 4. more sources than one launch
MANY_DIMS = (3, 2, 2)
MANY_EXTRA = 70


def many_sources():
    """(free, sources): 3 x 2 x 2 with voxel (1, 0, 0) occupied; MAX_CHUNK + 70 sources cycling through the 11 free voxels"""
    free = np.ones(12, np.uint8)
    free[1] = 0
    ids = np.flatnonzero(free)
    return free, ids[np.arange(MAX_CHUNK + MANY_EXTRA) % len(ids)].astype(np.int64)


# the rows of sources 65 534, 65 535 and 65 536 by hand.  Ids are x + 3 y + 6 z; 65 534 = 11 * 5957 + 7, so these are the 8th, 9th and
# 10th free voxel: ids 8 = (2, 0, 1), 9 = (0, 1, 1) and 10 = (1, 1, 1).  Voxel 1 = (1, 0, 0) is metal (-1): corner 0 = (0, 0, 0) is
# reached from (1, 1, *) through (0, 1, 0), never through (1, 0, 0), and from (2, 0, 1) the row y = 0, z = 1 leads to it, so every count
# below is the Manhattan distance except where the straight way would need voxel 1 -- there is none among these three rows.
MANY_BY_HAND = {
    65534: [3, -1, 1, 4, 3, 2, 2, 1, 0, 3, 2, 1],
    65535: [2, -1, 4, 1, 2, 3, 1, 2, 3, 0, 1, 2],
    65536: [3, -1, 3, 2, 1, 2, 2, 1, 2, 1, 0, 1],
}


def test_the_sources_split_at_the_launch_limit():
    free, src = many_sources()
    assert len(src) == 65535 + 70 > MAX_CHUNK and free.sum() == 11
    assert [int(src[s]) for s in (65534, 65535, 65536)] == [8, 9, 10]
    for s, row in MANY_BY_HAND.items():
        assert G.field(free, MANY_DIMS, int(src[s])).tolist() == row == G.queue_field(free, MANY_DIMS, int(src[s])).tolist()
    assert G.field(free, MANY_DIMS, 0).tolist() == [0, -1, 4, 1, 2, 3, 1, 2, 3, 2, 3, 4]       # the metal voxel lengthens (0,0,0) -> (2,0,0) to 4
