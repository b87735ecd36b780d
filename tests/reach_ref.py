"""numpy restatement of the torch-fit planning grids of include/weldacs.h (wa_grid_tool_reach, wa_grid_tool_fit,
wa_grid_tool_penalties; rules 10 - 15 of the torch section), written from the header's definition and independent of the kernels.
Built on torch_ref's quantise_all / offsets / beads and clearance_ref's distance field; it takes NO shortcut: every (voxel, direction,
bead) is looked up.  grid = (free, d2, dims, axes) as torch_ref.make_grid returns it."""
import math

import numpy as np

import torch_ref as TR

SUMMARY_FIELDS = ("n_free", "n_no_dir", "n_all_dirs", "n_blocked_pairs")


def voxels(dims):
    """(n, 3) voxel triples (x, y, z) in raster order"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int64)


def open_dirs(grid, dirs, tool):
    """open(v, k) as bool [n, K] (rule 10)"""
    free, _, dims, _ = grid
    dist16, r2 = tool
    q = TR.quantise_all(dirs)
    off = TR.offsets(q, dist16)                                # K, n_beads, 3
    vox = voxels(dims)
    n, K = len(vox), len(q)
    out = np.zeros((n, K), bool)
    step = max(1, (1 << 21) // max(1, K * len(dist16)))
    for s in range(0, n, step):
        b, _ = TR.beads(grid, vox[s:s + step, None, :], off[None], r2, -1)
        out[s:s + step] = ~b.any(-1)
    out &= (np.asarray(free).ravel() != 0)[:, None]
    return out


def pack(opened):
    """bool [n, K] -> uint64 [W, n], word-plane-major (rule 11)"""
    n, K = opened.shape
    W = (K + 63) // 64
    mask = np.zeros((W, n), np.uint64)
    for k in range(K):
        mask[k >> 6] |= opened[:, k].astype(np.uint64) << np.uint64(k & 63)
    return mask


def summarise(free, count, K):
    f = np.asarray(free).ravel() != 0
    c = count.astype(np.int64)
    return dict(n_free=int(f.sum()), n_no_dir=int((f & (c == 0)).sum()), n_all_dirs=int((f & (c == K)).sum()),
                n_blocked_pairs=int((K - c[f]).sum()))


def reach(grid, dirs, tool):
    """wa_grid_tool_reach: (mask uint64[W, n], count uint16[n], summary dict)"""
    opened = open_dirs(grid, dirs, tool)
    count = opened.sum(1).astype(np.uint16)
    return pack(opened), count, summarise(grid[0], count, opened.shape[1])


def fit(grid, dirs, tool, min_dirs=1, keep_ids=(), keep_r2=0, count=None):
    """wa_grid_tool_fit: the new occupancy (flat uint8, 1 = free); count: a reach() result to reuse"""
    free, _, dims, _ = grid
    free = (np.asarray(free).ravel() != 0)
    if count is None:
        count = reach(grid, dirs, tool)[1]
    K = len(np.asarray(dirs).reshape(-1, 3))
    assert 1 <= min_dirs <= K and keep_r2 >= 0
    out = free & (count.astype(np.int64) >= min_dirs)
    vox = voxels(dims)
    for k in keep_ids:
        assert 0 <= k < len(free) and free[k], "a keep id is a free voxel of the grid"
        d = vox - vox[int(k)]
        inside = (d * d).sum(1) <= keep_r2
        out[inside] = free[inside]
    return out.astype(np.uint8)


def penalties(grid, dirs, tool, thr, count=None):
    """wa_grid_tool_penalties: uint8 [n]"""
    free = np.asarray(grid[0]).ravel() != 0
    if count is None:
        count = reach(grid, dirs, tool)[1]
    thr = np.asarray(thr, np.int64).reshape(-1)
    assert len(thr) <= 31 and (len(thr) == 0 or (thr.min() >= 0 and thr.max() <= 65535))
    pen = (count.astype(np.int64)[:, None] < thr[None, :]).sum(1)
    return np.where(free, pen, 0).astype(np.uint8)


def prune_radius(tool):
    """R of the far-voxel shortcut: a free voxel with d2 >= R^2 has every direction open"""
    dist16, r2 = tool
    return max((int(d) + 15) // 16 + 2 + math.isqrt(int(r)) + 1 for d, r in zip(dist16, r2))


def far_near(grid, tool):
    """(far, near) bool [n]: the free voxels at or beyond prune_radius, and the other free voxels"""
    free, d2, _, _ = grid
    f = np.asarray(free).ravel() != 0
    far = f & (np.asarray(d2, np.int64).ravel() >= prune_radius(tool) ** 2)
    return far, f & ~far


# ---- scenes
def tunnel_scene():
    """a wall with a low tunnel: grid 40 x 24 x 28, metal at x 18 .. 21, z 0 .. 17, all y; a 3 x 3 tunnel at y 10 .. 12, z 2 .. 4.
    dict(grid, dirs, tool, start, end): a 10-bead rod of 10 voxels, a 32-direction cone of half angle 0.6 around +z."""
    nx, ny, nz = 40, 24, 28
    free = np.ones((nz, ny, nx), np.uint8)
    free[0:18, :, 18:22] = 0
    free[2:5, 10:13, 18:22] = 1
    idx = lambda x, y, z: (z * ny + y) * nx + x   # noqa: E731
    return dict(grid=TR.make_grid(free, (nx, ny, nz)), dirs=TR.fib_dirs(32, 0.6, (0.0, 0.0, 1.0)), tool=TR.rod(10, 160, 1),
                start=idx(4, 11, 3), end=idx(35, 11, 3))


def box_scene(seed, m=24):
    """a seeded m^3 box scene with both far and near free voxels for a short rod; (grid, dirs, tool)"""
    rs = np.random.RandomState(7000 + seed)
    free = np.ones((m, m, m), np.uint8)
    for _ in range(int(rs.randint(2, 5))):
        lo = rs.randint(0, m // 3, 3)
        sz = rs.randint(1, max(2, m // 6), 3)
        free[lo[2]:lo[2] + sz[2], lo[1]:lo[1] + sz[1], lo[0]:lo[0] + sz[0]] = 0
    tool = TR.rod(int(rs.randint(2, 6)), int(rs.randint(16, 16 * 4)), int(rs.randint(0, 3)))
    dirs = TR.fib_dirs(int(rs.choice([5, 16, 33])), float(rs.uniform(0.4, 2.6)), rs.normal(size=3))
    return TR.make_grid(free, (m, m, m)), dirs, tool
