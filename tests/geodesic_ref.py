"""numpy restatement of the exact shortest-path fields, written from the definitions in include/weldacs.h alone (section "exact
shortest-path fields"): hop counts by a frontier breadth-first search on boolean arrays, and the walk-back rule that defines THE path.
Imports numpy only, so worker processes that use it never open the GPU."""
import numpy as np

NONE = -1   # WA_HOPS_NONE


def field(free, dims, src):
    """hops(src, v) for every voxel v as a flat int32 array in raster order; free: flat uint8, != 0 = free; dims = (nx, ny, nz)"""
    nx, ny, nz = dims
    f3 = np.asarray(free).reshape(nz, ny, nx) != 0
    hops = np.full((nz, ny, nx), NONE, np.int32)
    z, y, x = int(src) // (nx * ny), (int(src) // nx) % ny, int(src) % nx
    assert f3[z, y, x], "an occupied source is an argument error"
    fr = np.zeros_like(f3)
    fr[z, y, x] = True
    hops[z, y, x] = 0
    seen = fr.copy()
    level = 0
    while True:
        nxt = np.zeros_like(fr)
        nxt[:, :, 1:] |= fr[:, :, :-1]
        nxt[:, :, :-1] |= fr[:, :, 1:]
        nxt[:, 1:, :] |= fr[:, :-1, :]
        nxt[:, :-1, :] |= fr[:, 1:, :]
        nxt[1:] |= fr[:-1]
        nxt[:-1] |= fr[1:]
        nxt &= f3
        nxt &= ~seen
        if not nxt.any():
            return hops.reshape(-1)
        level += 1
        hops[nxt] = level
        seen |= nxt
        fr = nxt


def fields(free, dims, srcs):
    return np.stack([field(free, dims, s) for s in srcs]) if len(srcs) else np.zeros((0, int(np.prod(dims))), np.int32)


def matrix(free, dims, pts):
    pts = np.asarray(pts, np.int64)
    return np.stack([field(free, dims, s)[pts] for s in pts]).astype(np.int32) if len(pts) else np.zeros((0, 0), np.int32)


def neighbours(v, dims):
    """the neighbours of voxel v that lie inside the grid, in the fixed order -x, +x, -y, +y, -z, +z"""
    nx, ny, nz = dims
    x, y, z = v % nx, (v // nx) % ny, v // (nx * ny)
    out = []
    if x > 0:
        out.append(v - 1)
    if x < nx - 1:
        out.append(v + 1)
    if y > 0:
        out.append(v - nx)
    if y < ny - 1:
        out.append(v + nx)
    if z > 0:
        out.append(v - nx * ny)
    if z < nz - 1:
        out.append(v + nx * ny)
    return out


def walk_back(hops, dims, end):
    """the path start -> end given hops = field(free, dims, start): None when end is not reachable"""
    k = int(hops[end])
    if k < 0:
        return None
    v = int(end)
    path = [v]
    while k > 0:
        v = next(n for n in neighbours(v, dims) if hops[n] == k - 1)   # (a voxel with a hop count is free)
        path.append(v)
        k -= 1
    return np.array(path[::-1], np.int64)


def paths(free, dims, starts, ends):
    """(hops int32[n], [path or None])"""
    cache, hops, out = {}, [], []
    for s, e in zip(starts, ends):
        s, e = int(s), int(e)
        if s not in cache:
            cache[s] = field(free, dims, s)
        hops.append(int(cache[s][e]))
        out.append(walk_back(cache[s], dims, e))
    return np.array(hops, np.int32), out


def queue_field(free, dims, src):
    """an independent check of field(): a plain first-in first-out queue"""
    from collections import deque
    free = np.asarray(free).reshape(-1)
    hops = np.full(free.size, NONE, np.int32)
    hops[src] = 0
    q = deque([int(src)])
    while q:
        v = q.popleft()
        for n in neighbours(v, dims):
            if free[n] and hops[n] < 0:
                hops[n] = hops[v] + 1
                q.append(n)
    return hops


def check_path(free, dims, path, start, end, hops):
    """what a shortest path must satisfy whichever rule picked it: start first, end last, hops + 1 ids, every step a 6-neighbour step
    between free voxels"""
    free = np.asarray(free).reshape(-1)
    path = np.asarray(path, np.int64)
    assert len(path) == hops + 1 and path[0] == start and path[-1] == end
    assert (free[path] != 0).all()
    for a, b in zip(path[:-1].tolist(), path[1:].tolist()):
        assert b in neighbours(a, dims), (a, b)


def serpentine(nx, ny):
    """free bytes of an nx x ny x 1 grid: a wall on every second row (y odd) with a one-voxel gap at alternating ends; the corridor from
    voxel 0 visits every free voxel in turn"""
    f = np.ones((ny, nx), np.uint8)
    for k, y in enumerate(range(1, ny, 2)):
        f[y, :] = 0
        f[y, nx - 1 if k % 2 == 0 else 0] = 1
    return f.reshape(-1)


def baffles(nx, ny, nz, every=3):
    """free bytes of a box with walls across it at x = every - 1, 2 * every - 1, ... , each with one gap at alternating corners"""
    f = np.ones((nz, ny, nx), np.uint8)
    for k, x in enumerate(range(every - 1, nx - 1, every)):
        f[:, :, x] = 0
        if k % 2 == 0:
            f[0, 0, x] = 1
        else:
            f[nz - 1, ny - 1, x] = 1
    return f.reshape(-1)


def hand_cases():
    """(name, free, dims, source, {voxel: hops}) -- answers worked out by hand from the definition"""
    cases = []
    nx = ny = nz = 3
    idx = lambda x, y, z, nx=3, ny=3: x + nx * (y + ny * z)
    cases.append(("empty_box_is_manhattan", np.ones(27, np.uint8), (3, 3, 3), idx(0, 0, 0),
                  {idx(x, y, z): x + y + z for x in range(3) for y in range(3) for z in range(3)}))
    cases.append(("empty_box_from_the_centre", np.ones(27, np.uint8), (3, 3, 3), idx(1, 1, 1),
                  {idx(x, y, z): abs(x - 1) + abs(y - 1) + abs(z - 1) for x in range(3) for y in range(3) for z in range(3)}))
    # 5 x 3 x 1, a wall at x = 2 with its one hole at y = 2
    f = np.ones((3, 5), np.uint8)
    f[:, 2] = 0
    f[2, 2] = 1
    i51 = lambda x, y: x + 5 * y
    cases.append(("wall_with_one_hole", f.reshape(-1), (5, 3, 1), i51(0, 0),
                  {i51(1, 0): 1, i51(0, 2): 2, i51(2, 2): 4, i51(3, 2): 5, i51(3, 0): 7, i51(4, 0): 8, i51(2, 0): NONE, i51(2, 1): NONE}))
    # 5 x 5 x 1 with the centre free inside a ring of its four occupied neighbours
    f = np.ones((5, 5), np.uint8)
    for x, y in ((1, 2), (3, 2), (2, 1), (2, 3)):
        f[y, x] = 0
    i55 = lambda x, y: x + 5 * y
    cases.append(("enclosed_free_voxel", f.reshape(-1), (5, 5, 1), i55(0, 0),
                  {i55(2, 2): NONE, i55(1, 2): NONE, i55(4, 4): 8, i55(1, 1): 2, i55(2, 0): 2}))
    return cases


def tie_case():
    """2 x 2 x 2, all free, from voxel 0 to voxel 7 = (1, 1, 1): its three predecessors (0,1,1), (1,0,1), (1,1,0) all have hop count 2 and
    -x comes first, and so on down: the path is 0 -> (0,0,1) -> (0,1,1) -> (1,1,1) = ids 0, 4, 6, 7"""
    return np.ones(8, np.uint8), (2, 2, 2), 0, 7, [0, 4, 6, 7]


def bellman_exact(hops, free, dims, src, slab=32):
    """True iff hops is THE hop field of src: hops[src] = 0; no other voxel has 0; every voxel with a count k > 0 is free and the smallest
    count among its neighbours that have one is k - 1; no free voxel without a count has a neighbour with one.  That pins the field down:
    following smallest neighbours from a voxel with count k reaches the only 0, the source, in k steps, so k >= the distance; and
    k <= 1 + the count of every neighbour gives k <= the distance by induction along a shortest path."""
    nx, ny, nz = dims
    h3 = hops.reshape(nz, ny, nx)
    f3 = free.reshape(nz, ny, nx) != 0
    BIG = np.int32(2 ** 30)
    if hops[src] != 0 or (hops == 0).sum() != 1 or (hops[free == 0] != NONE).any():
        return False
    for z0 in range(0, nz, slab):
        z1 = min(nz, z0 + slab)
        a, b = max(z0 - 1, 0), min(z1 + 1, nz)
        big = np.where(h3[a:b] >= 0, h3[a:b], BIG)
        lo = np.full_like(big, BIG)
        np.minimum(lo[:, :, 1:], big[:, :, :-1], out=lo[:, :, 1:])
        np.minimum(lo[:, :, :-1], big[:, :, 1:], out=lo[:, :, :-1])
        np.minimum(lo[:, 1:, :], big[:, :-1, :], out=lo[:, 1:, :])
        np.minimum(lo[:, :-1, :], big[:, 1:, :], out=lo[:, :-1, :])
        np.minimum(lo[1:], big[:-1], out=lo[1:])
        np.minimum(lo[:-1], big[1:], out=lo[:-1])
        lo, h, f = lo[z0 - a:z0 - a + (z1 - z0)], h3[z0:z1], f3[z0:z1]
        if not np.array_equal(lo[h > 0] + 1, h[h > 0]):
            return False
        if (lo[f & (h < 0)] != BIG).any():
            return False
    return True


GOLDEN_256_SOURCES = (0, 21, 42, 63)   # which of C5's 64 weld points tests/golden/geodesic_c5_rows.json holds rows for


def _golden_row(i):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from welding_robot_amd import synth
    free = synth.synth_grid(256)[0]
    pts = synth.synth_weld_points(free, 256, 64)
    return field(free, (256, 256, 256), pts[i])[pts].tolist()


if __name__ == "__main__":
    # python tests/geodesic_ref.py: rewrites the golden rows of the full-size matrix test from this restatement (minutes of numpy; the
    # GPU test only reads them)
    import json
    import multiprocessing as mp
    import os
    with mp.Pool(len(GOLDEN_256_SOURCES)) as pool:
        rows = pool.map(_golden_row, GOLDEN_256_SOURCES)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_c5_rows.json")
    with open(out, "w") as f:
        json.dump({"grid": 256, "points": 64, "sources": list(GOLDEN_256_SOURCES), "rows": rows}, f)
        f.write("\n")
    print(out)
