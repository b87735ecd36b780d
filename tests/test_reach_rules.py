"""The restatement of the torch-fit planning grids (tests/reach_ref.py) held against a brute force that never looks at the distance
field, the far-voxel bound of DESIGN 4s on seeded scenes, and hand cases.  CPU only: no library call here."""
import numpy as np
import pytest

import reach_ref as RR
import torch_ref as TR


def brute_open(free, dims, dirs, tool):
    """open(v, k) from the occupancy alone: a bead at voxel b is blocked iff some occupied voxel u has |b - u|^2 <= r2"""
    nx, ny, nz = dims
    dist16, r2 = tool
    q = TR.quantise_all(dirs)
    K, nb = len(q), len(dist16)
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    occ = np.argwhere(~f3)[:, ::-1].astype(np.int64)           # (x, y, z) of every occupied voxel
    out = np.zeros((nx * ny * nz, K), bool)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                if not f3[z, y, x]:
                    continue
                for k in range(K):
                    ok = True
                    for j in range(nb):
                        o = [(int(q[k, c]) * int(dist16[j]) + (1 << 17)) // (1 << 18) for c in range(3)]
                        b = np.array([x + o[0], y + o[1], z + o[2]], np.int64)
                        if not (0 <= b[0] < nx and 0 <= b[1] < ny and 0 <= b[2] < nz):
                            continue
                        if len(occ) and (((occ - b) ** 2).sum(1) <= int(r2[j])).any():
                            ok = False
                            break
                    out[(z * ny + y) * nx + x, k] = ok
    return out


@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_brute_force_without_the_distance_field(seed):
    rs = np.random.RandomState(100 + seed)
    dims = (9, 8, 7)
    free = (rs.uniform(size=dims[::-1]) > 0.08).astype(np.uint8)
    K = int(rs.randint(3, 7))
    dirs = rs.normal(size=(K, 3)).astype(np.float32)
    nb = int(rs.randint(1, 5))
    tool = (np.sort(rs.randint(0, 16 * 7, nb)).astype(np.int64), rs.randint(0, 4, nb).astype(np.int64))
    grid = TR.make_grid(free, dims)
    want = brute_open(free, dims, dirs, tool)
    mask, count, summary = RR.reach(grid, dirs, tool)
    assert np.array_equal(RR.open_dirs(grid, dirs, tool), want)
    assert np.array_equal(count, want.sum(1).astype(np.uint16))
    for k in range(K):
        assert np.array_equal((mask[k >> 6] >> np.uint64(k & 63)) & np.uint64(1), want[:, k].astype(np.uint64))
    f = free.ravel() != 0
    assert summary == dict(n_free=int(f.sum()), n_no_dir=int((f & (count == 0)).sum()), n_all_dirs=int((f & (count == K)).sum()),
                           n_blocked_pairs=int((K - count[f].astype(np.int64)).sum()))
    assert 0 < summary["n_blocked_pairs"] < K * summary["n_free"]    # the scene decides something


@pytest.mark.parametrize("seed", range(7))
def test_far_voxels_have_every_direction_open(seed):
    grid, dirs, tool = RR.box_scene(seed)
    K = len(dirs)
    far, near = RR.far_near(grid, tool)
    assert far.any() and near.any(), "a scene needs far and near free voxels"
    _, count, _ = RR.reach(grid, dirs, tool)
    assert (count[far] == K).all()
    assert (count[near] < K).any()                             # ... and the near set is where directions close


def test_prune_radius_is_the_formula():
    assert RR.prune_radius(([0], [0])) == 0 + 2 + 0 + 1
    assert RR.prune_radius(([160, 17], [1, 9])) == max(10 + 2 + 1 + 1, 2 + 2 + 3 + 1)
    assert RR.prune_radius(([65536], [1 << 30])) == 4096 + 2 + 32768 + 1
    assert RR.prune_radius(([65536], [1 << 30])) ** 2 < 2 ** 31


def test_empty_and_full_grids():
    dims = (6, 5, 4)
    dirs, tool = TR.fib_dirs(70, 1.0), TR.rod(4, 48, 2)
    n = int(np.prod(dims))
    mask, count, s = RR.reach(TR.make_grid(np.ones(n, np.uint8), dims), dirs, tool)
    assert (count == 70).all() and s == dict(n_free=n, n_no_dir=0, n_all_dirs=n, n_blocked_pairs=0)
    assert (mask[0] == np.uint64(2 ** 64 - 1)).all() and (mask[1] == np.uint64(2 ** 6 - 1)).all()   # unused high bits are 0
    mask, count, s = RR.reach(TR.make_grid(np.zeros(n, np.uint8), dims), dirs, tool)
    assert (count == 0).all() and not mask.any() and s == dict(n_free=0, n_no_dir=0, n_all_dirs=0, n_blocked_pairs=0)


def test_bead_on_the_tip_next_to_metal():
    """one bead at distance 0: it sits on the voxel itself, whose d2 is 1 next to metal.  r2 = 0 passes (1 > 0), r2 = 1 blocks."""
    dims = (5, 1, 1)
    free = np.array([1, 1, 0, 1, 1], np.uint8)
    grid = TR.make_grid(free, dims)
    dirs = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    _, c0, s0 = RR.reach(grid, dirs, ([0], [0]))
    assert c0.tolist() == [2, 2, 0, 2, 2] and s0["n_no_dir"] == 0
    _, c1, s1 = RR.reach(grid, dirs, ([0], [1]))
    assert c1.tolist() == [2, 0, 0, 0, 2] and s1 == dict(n_free=4, n_no_dir=2, n_all_dirs=2, n_blocked_pairs=4)
    assert RR.fit(grid, dirs, ([0], [1])).tolist() == [1, 0, 0, 0, 1]
    assert RR.fit(grid, dirs, ([0], [1]), keep_ids=[1], keep_r2=0).tolist() == [1, 1, 0, 0, 1]
    assert RR.fit(grid, dirs, ([0], [1]), keep_ids=[1], keep_r2=4).tolist() == [1, 1, 0, 1, 1]
    assert RR.penalties(grid, dirs, ([0], [1]), [1, 3, 1, 0]).tolist() == [1, 3, 0, 3, 1]


def test_tool_longer_than_the_grid_passes():
    """every bead lands outside the grid, so nothing is blocked although the grid is mostly metal"""
    dims = (4, 4, 4)
    free = np.zeros(dims, np.uint8)
    free[1, 2, 1] = free[2, 2, 2] = 1
    dirs = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, -1, -1]], np.float32)
    tool = ([16 * 9, 16 * 20, 65536], [5, 5, 5])
    _, count, s = RR.reach(TR.make_grid(free, dims), dirs, tool)
    assert count.sum() == 8 and s == dict(n_free=2, n_no_dir=0, n_all_dirs=2, n_blocked_pairs=0)


def test_tunnel_scene_numbers():
    """what the feature is for: the hop-optimal path runs through a tunnel where the torch has no direction; on the fit grid it goes
    over the wall"""
    import geodesic_ref as GR
    sc = RR.tunnel_scene()
    grid = sc["grid"]
    free, _, dims, _ = grid
    _, count, _ = RR.reach(grid, sc["dirs"], sc["tool"])
    hops = GR.field(free, dims, sc["start"])
    path = GR.walk_back(hops, dims, sc["end"])
    assert len(path) - 1 == 31 and int((count[path] == 0).sum()) == 4
    fit = RR.fit(grid, sc["dirs"], sc["tool"], 1, count=count)
    path2 = GR.walk_back(GR.field(fit, dims, sc["start"]), dims, sc["end"])
    assert len(path2) - 1 == 63 and int((count[path2] == 0).sum()) == 0
