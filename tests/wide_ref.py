"""Oracle runs for tests/test_gpu_wide_batches.py, in worker processes.

A wide batch is hundreds of searches, and the oracle runs one search per CPU core.  The GPU test farms them out to a
pool of `spawn`ed workers that execute this module.  It imports numpy and oracle_lib only -- never the package's api or
torch -- so no worker ever opens the GPU.

A task names its grid by a small spec (rebuilt once per worker) and returns what the test compares: the per-generation
trace, the last generation's ants, the best cost and path, and a digest of the whole pheromone field's bits (a field of
48^3 voxels is 2.6 MB; a digest lets every search's field be compared without holding hundreds of them)."""
import hashlib

import numpy as np

import oracle_lib as O

_grids = {}


def grid(spec):
    """spec = ("synth", n, seed, occ_prob, walls): O.synth_grid with the voxels listed in `walls` made occupied;
    ("box", (nx, ny, nz), seed, occ_prob, walls): unit voxels, occupied where a numpy RandomState(seed) uniform is < occ_prob"""
    if spec not in _grids:
        kind, n, seed, occ, walls = spec
        if kind == "synth":
            g = O.synth_grid(n, seed=seed, occ_prob=occ)
        else:
            assert kind == "box"
            nx, ny, nz = n
            free = (np.random.RandomState(seed).uniform(size=nx * ny * nz) >= occ).astype(np.uint8)
            g = O.Grid(np.arange(nx, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nz, dtype=np.float32), free, 1.0, 0)
        for v in walls:
            g.free[v] = 0
        _grids[spec] = g
    return _grids[spec]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def field_digest(field):
    return hashlib.blake2b(bits(field).tobytes(), digest_size=16).hexdigest()


def run_one(task):
    """task = (grid spec, start, end, generations, predict, fixed colony, seed, stream, neighbours, reset): a fresh field as
    initFromGridMap leaves it (out-of-bounds edges 0), or with `reset` as reset(1.0) leaves it (every edge 1)"""
    spec, start, end, iters, predict, ants, seed, stream, nb, reset = task
    a = O.Acs(grid(spec), nb=nb)
    if reset:
        a.reset(1.0)
    tr = a.solve(start, end, iters, predict, fixed_colony=ants, mode=O.DEV, seed=seed, stream=stream)
    lens, L = a.last_ants()
    return dict(steps=tr["steps"].copy(), finite=tr["finite"].copy(), bestL=bits(tr["bestL"]).copy(), colony=tr["colony"].copy(),
                antL=bits(L).copy(), antlen=lens.copy(), cost=bits(a.best_L).copy(), path=a.best_path()[0].copy(),
                field=field_digest(a.pheromone()))
