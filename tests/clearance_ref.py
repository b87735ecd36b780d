"""numpy restatements of the clearance entry points of include/weldacs.h (wa_grid_distance_field, wa_grid_inflate,
wa_traj_clearance), written from the header's definitions and independent of the kernels' algorithms."""
import numpy as np

D2_NONE = 0x7FFFFFFF


def _shape(nx, ny, nz):
    return (nz, ny, nx)


def edt_brute(free, nx, ny, nz):
    """min over occupied voxels of the squared index distance, by brute force (small grids)"""
    f3 = np.asarray(free, np.uint8).reshape(_shape(nx, ny, nz))
    occ = np.argwhere(f3 == 0).astype(np.int64)          # (z, y, x)
    if len(occ) == 0:
        return np.full(nx * ny * nz, D2_NONE, np.int32)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], 1).astype(np.int64)
    out = np.full(len(pts), np.iinfo(np.int64).max, np.int64)
    for s in range(0, len(occ), 256):
        o = occ[s:s + 256]
        d = ((pts[:, None, :] - o[None, :, :]) ** 2).sum(-1).min(1)
        out = np.minimum(out, d)
    return out.astype(np.int32)


def _axis_pass(f, axis):
    """g(j) = min_i f(i) + (j - i)^2 along `axis` (int64, INF = no obstacle in the line), by offsets of growing size that stop once
    the offset alone exceeds every value still able to change"""
    INF = np.iinfo(np.int64).max // 4
    n = f.shape[axis]
    out = f.copy()
    has = (f < INF).any(axis=axis, keepdims=True) & np.ones_like(f, bool)
    for dlt in range(1, n):
        blocking = out[has]
        if blocking.size == 0 or dlt * dlt > blocking.max():
            break
        sq = dlt * dlt
        a = [slice(None)] * f.ndim
        b = [slice(None)] * f.ndim
        # from the left neighbour at distance dlt, and from the right one
        a[axis], b[axis] = slice(dlt, None), slice(None, n - dlt)
        out[tuple(a)] = np.minimum(out[tuple(a)], f[tuple(b)] + sq)
        out[tuple(b)] = np.minimum(out[tuple(b)], f[tuple(a)] + sq)
    return out


def edt_separable(free, nx, ny, nz):
    """the same field by three 1-D passes (exact: the squared distance splits into its axes)"""
    INF = np.iinfo(np.int64).max // 4
    f3 = np.asarray(free, np.uint8).reshape(_shape(nx, ny, nz))
    f = np.where(f3 == 0, 0, INF).astype(np.int64)
    for axis in (2, 1, 0):
        f = _axis_pass(f, axis)
        f = np.minimum(f, INF)
    return np.where(f >= INF, D2_NONE, f).astype(np.int32).ravel()


def inflate(free, d2, nx, ny, nz, radius, keep_ids=()):
    free = np.asarray(free, np.uint8).ravel()
    d2 = np.asarray(d2, np.int32).ravel()
    r2 = float(np.float32(radius)) ** 2
    out = (free.astype(bool) & ((d2 == D2_NONE) | (d2.astype(np.float64) > r2))).astype(np.uint8)
    rk2 = (float(np.float32(radius)) + 1.0) ** 2
    if len(keep_ids):
        zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        xx, yy, zz = xx.ravel(), yy.ravel(), zz.ravel()
        for k in keep_ids:
            k = int(k)
            kx, ky, kz = k % nx, (k // nx) % ny, k // (nx * ny)
            m = ((xx - kx) ** 2 + (yy - ky) ** 2 + (zz - kz) ** 2).astype(np.float64) <= rk2
            out[m] = free[m]
    return out


def axis_node(c, p):
    """lowest j minimising |p - c[j]| (fp32) after clamping p into [min c, max c] (NaN to min); returns (j, outside)"""
    c = np.asarray(c, np.float32)
    lo, hi = c.min(), c.max()
    p = np.float32(p)
    outside = False
    if not (p >= lo):
        p, outside = lo, True
    elif p > hi:
        p, outside = hi, True
    return int(np.argmin(np.abs(p - c))), outside


def supercover(a, b):
    """voxels (x, y, z) of the supercover between voxels a and b, by the header's rule: v is in it iff [0, 1] and the per-axis sets
    of t share a point; integer comparisons only (t = num / den with den > 0)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    d = b - a
    ranges = [range(min(a[c], b[c]), max(a[c], b[c]) + 1) for c in range(3)]
    out = []
    for x in ranges[0]:
        for y in ranges[1]:
            for z in ranges[2]:
                v = (x, y, z)
                lo_n, lo_d, hi_n, hi_d = 0, 1, 1, 1        # [lo, hi] = [0, 1]
                ok = True
                for c in range(3):
                    if d[c] == 0:
                        if v[c] != a[c]:
                            ok = False
                        continue
                    e1, e2 = 2 * (v[c] - a[c]) - 1, 2 * (v[c] - a[c]) + 1
                    den = 2 * abs(int(d[c]))
                    if d[c] < 0:
                        e1, e2 = -e2, -e1
                    # lo = max(lo, e1/den), hi = min(hi, e2/den)
                    if e1 * lo_d > lo_n * den:
                        lo_n, lo_d = e1, den
                    if e2 * hi_d < hi_n * den:
                        hi_n, hi_d = e2, den
                if ok and lo_n * hi_d <= hi_n * lo_d:
                    out.append(v)
    return out


def clearance(free, d2, nx, ny, nz, cx, cy, cz, xyz):
    """(ids, d2, hits, summary) of wa_traj_clearance"""
    free = np.asarray(free, np.uint8).ravel()
    d2 = np.asarray(d2, np.int32).ravel()
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    ids = np.empty(n, np.int64)
    vox = []
    n_out = 0
    for i in range(n):
        x, ox = axis_node(cx, xyz[i, 0])
        y, oy = axis_node(cy, xyz[i, 1])
        z, oz = axis_node(cz, xyz[i, 2])
        n_out += ox or oy or oz
        vox.append((x, y, z))
        ids[i] = (z * ny + y) * nx + x
    sd = d2[ids] if n else np.zeros(0, np.int32)
    hits = np.zeros(max(n - 1, 0), np.uint8)
    for i in range(n - 1):
        hits[i] = any(free[(v[2] * ny + v[1]) * nx + v[0]] == 0 for v in supercover(vox[i], vox[i + 1]))
    summ = {"min_d2": int(sd.min()) if n else D2_NONE, "argmin": int(np.argmin(sd)) if n else -1,
            "first_hit": int(np.flatnonzero(hits)[0]) if hits.any() else -1, "n_hit": int(hits.sum()), "n_outside": int(n_out)}
    return ids, sd.astype(np.int32), hits, summ


def shuffled_scene():
    """a 23 x 17 x 11 grid with 8 % metal whose tables take every path of the lookup -- x stretched, y shuffled (not monotone: the
    scan), z with a duplicated last node, as at a seam -- and 300 samples on nodes, between them and outside.
    Returns (free, dims, (cx, cy, cz), xyz)."""
    rs = np.random.RandomState(9)
    nx, ny, nz = 23, 17, 11
    free = (rs.uniform(size=nx * ny * nz) >= 0.08).astype(np.uint8)
    cx = (np.arange(nx) * 0.25 - 1).astype(np.float32)
    cy = rs.permutation(np.arange(ny)).astype(np.float32) * np.float32(0.5)
    cz = np.concatenate([np.arange(nz - 1), [nz - 2]]).astype(np.float32)
    xyz = np.stack([rs.uniform(-1.5, 5, 300), rs.uniform(-1, 9, 300), rs.uniform(-1, 11, 300)], 1).astype(np.float32)
    xyz[::7] = np.stack([cx[rs.randint(0, nx, len(xyz[::7]))], cy[rs.randint(0, ny, len(xyz[::7]))], cz[rs.randint(0, nz, len(xyz[::7]))]], 1)
    return free, (nx, ny, nz), (cx, cy, cz), xyz
