"""Oracle runs for tests/test_gpu_grid_limits.py, in worker processes.

The grids there are the largest the library accepts (up to 2^27 voxels; a 26-neighbour field of that size is 14 GB), so a task
returns the pheromone field as digests of fixed-size chunks, computed on the oracle's own array without copying it.  This module
imports numpy and oracle_lib only -- never the package's api or torch -- so no worker ever opens the GPU."""
import hashlib

import numpy as np

import oracle_lib as O

CHUNK = 1 << 24         # floats per field digest (64 MB)
_grids = {}


def box_free(dims, seed, occ, opens):
    """occupancy of a (nx, ny, nz) box grid: occupied where a uniform draw is < occ, drawn one z-slab at a time from
    RandomState(seed + z); the voxel ids in `opens` free"""
    nx, ny, nz = dims
    nxy = nx * ny
    free = np.empty(nxy * nz, np.uint8)
    for z in range(nz):
        free[z * nxy:(z + 1) * nxy] = np.random.RandomState(seed + z).uniform(size=nxy) >= occ
    free[list(opens)] = 1
    return free


def grid(spec):
    """spec = (dims, seed, occ, opens): unit voxels, precision 1, wall 0"""
    if spec not in _grids:
        _grids.clear()          # (one grid per worker at a time: the largest are 134 MB)
        dims, seed, occ, opens = spec
        ax = [np.arange(d, dtype=np.float32) for d in dims]
        _grids[spec] = O.Grid(ax[0], ax[1], ax[2], box_free(dims, seed, occ, opens), 1.0, 0)
    return _grids[spec]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def field_digests(field):
    """blake2b of each CHUNK floats of a field (any float32 array, read in place)"""
    return [hashlib.blake2b(memoryview(field[i:i + CHUNK]).cast("B"), digest_size=16).hexdigest() for i in range(0, len(field), CHUNK)]


def run_one(task):
    """task = (grid spec, start, end, generations, colony, seed, stream, neighbours, mode): a fixed colony, predict = colony / 0.35;
    mode "dev" (counter-based draws keyed by seed and stream) or "ref" (srand(seed))"""
    spec, start, end, gens, colony, seed, stream, nb, mode = task
    g = grid(spec)
    a = O.Acs(g, nb=nb)
    if mode == "dev":
        tr = a.solve(start, end, gens, colony / 0.35, fixed_colony=colony, mode=O.DEV, seed=seed, stream=stream)
    else:
        tr = a.solve(start, end, gens, colony / 0.35, fixed_colony=colony, mode=O.REF, rng=O.srand(seed))
    lens, L = a.last_ants()
    field = np.ctypeslib.as_array(O.lib().wo_acs_pheromone(a.h), shape=(g.n * nb,))
    out = dict(steps=tr["steps"].copy(), finite=tr["finite"].copy(), bestL=bits(tr["bestL"]).copy(), colony=tr["colony"].copy(),
               antL=bits(L).copy(), antlen=lens.copy(), cost=bits(a.best_L).copy(), path=a.best_path()[0].copy(),
               field=field_digests(field))
    del field
    a.__del__()
    return out
