"""numpy restatement of wa_grid_path_shortcut (include/weldacs.h): the greedy line-of-sight shortcut with prefix visibility and its float64
length, written from the header's definition and independent of the kernels (visibility is clearance_ref.supercover)."""
import numpy as np

import clearance_ref as CR


def voxel(v, nx, ny):
    v = int(v)
    return (v % nx, (v // nx) % ny, v // (nx * ny))


def visible(free, nx, ny, a, b):
    """no voxel of the supercover between node ids a and b is occupied (voxel a included)"""
    free = np.asarray(free).ravel()
    return all(free[(z * ny + y) * nx + x] != 0 for x, y, z in CR.supercover(voxel(a, nx, ny), voxel(b, nx, ny)))


def waypoints(free, nx, ny, path, max_span, cache=None):
    """indices into `path` of the greedy shortcut's waypoints (cache: an optional dict of visibility answers for this grid, shared
    between calls)"""
    cache = {} if cache is None else cache

    def vis(a, b):
        key = (int(a), int(b))
        if key not in cache:
            cache[key] = visible(free, nx, ny, a, b)
        return cache[key]

    path = np.asarray(path, np.int64).reshape(-1)
    L = len(path)
    if L == 0:
        return np.zeros(0, np.int64)
    out = [0]
    a = 0
    while a < L - 1:
        top = min(a + max_span, L - 1)
        j = a
        for k in range(a + 1, top + 1):      # prefix visibility: stop at the first candidate that is not visible
            if not vis(path[a], path[k]):
                break
            j = k
        a = j if j > a else a + 1
        out.append(a)
    return np.asarray(out, np.int64)


def length(nodes, nx, ny, cx, cy, cz):
    """sum over consecutive nodes of sqrt(dx^2 + dy^2 + dz^2): float64 on the fp32 tables, (dx*dx + dy*dy) + dz*dz, in order"""
    total = 0.0
    prev = None
    for v in np.asarray(nodes, np.int64).reshape(-1):
        x, y, z = voxel(v, nx, ny)
        q = (float(np.float32(cx[x])), float(np.float32(cy[y])), float(np.float32(cz[z])))
        if prev is not None:
            dx, dy, dz = q[0] - prev[0], q[1] - prev[1], q[2] - prev[2]
            total += float(np.sqrt(np.float64(dx * dx + dy * dy + dz * dz)))
        prev = q
    return total


def shortcut(free, nx, ny, cx, cy, cz, path, max_span, cache=None):
    """(waypoint indices into path, length of the shortened path)"""
    w = waypoints(free, nx, ny, path, max_span, cache)
    return w, length(np.asarray(path, np.int64)[w], nx, ny, cx, cy, cz)


def _id(x, y, z, nx, ny):
    return (z * ny + y) * nx + x


def hand_cases():
    """[(name, free, (nx, ny, nz), path node ids, max_span, expected waypoint indices)] on unit-spaced grids"""
    out = []
    n = 8
    free = np.ones(n ** 3, np.uint8)
    stair, p = [], [0, 0, 0]
    for s in range(15):                                   # x, y, z, x, y, z, ...: a 6-neighbour staircase to (5, 5, 5)
        stair.append(_id(*p, n, n))
        p[s % 3] += 1
    stair.append(_id(*p, n, n))
    out.append(("staircase_open_space", free, (n, n, n), stair, 128, [0, len(stair) - 1]))
    # an L around a block: x, y in 1..4 occupied (one layer); down the free column x = 0, then along the free row y = 0
    nx, ny = 6, 6
    fl = np.ones(nx * ny, np.uint8)
    for x in range(1, 5):
        for y in range(1, 5):
            fl[_id(x, y, 0, nx, ny)] = 0
    ell = [_id(0, y, 0, nx, ny) for y in range(4, -1, -1)] + [_id(x, 0, 0, nx, ny) for x in range(1, 5)]
    out.append(("l_keeps_corner", fl, (nx, ny, 1), ell, 128, [0, 4, 8]))
    out.append(("one_node", free, (n, n, n), [_id(3, 2, 1, n, n)], 128, [0]))
    out.append(("two_nodes", free, (n, n, n), [_id(3, 2, 1, n, n), _id(3, 3, 1, n, n)], 128, [0, 1]))
    a, b = _id(1, 1, 1, n, n), _id(2, 1, 1, n, n)
    out.append(("repeated_nodes", free, (n, n, n), [a, a, a, b, b, _id(3, 1, 1, n, n)], 128, [0, 5]))
    # 26-neighbour diagonals in the xy plane past the occupied (1, 0, 0): the supercover of (0,0) -> (1,1) holds it
    fd = np.ones(n ** 3, np.uint8)
    fd[_id(1, 0, 0, n, n)] = 0
    out.append(("diagonal_grazes_edge", fd, (n, n, n), [_id(k, k, 0, n, n) for k in range(4)], 128, [0, 1, 3]))
    # a path that starts on an occupied voxel: nothing is visible from it
    out.append(("occupied_start", fd, (n, n, n), [_id(1, 0, 0, n, n), _id(2, 0, 0, n, n), _id(3, 0, 0, n, n)], 128, [0, 1, 2]))
    out.append(("span_1_is_the_input", free, (n, n, n), stair, 1, list(range(len(stair)))))
    out.append(("span_4", free, (n, n, n), stair, 4, [0, 4, 8, 12, 15]))
    return out
