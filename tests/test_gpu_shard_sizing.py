"""Shard sizing for the pair loop (SURVEY 8(e) partitioning; ACSRank_3D.hpp:472-499 runs the searches one after another):
wa_acs_memory_estimate against what the allocator really hands out, and the slot rule at BASELINE config C5's shape."""
import os

import numpy as np
import pytest

from welding_robot_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lazy,colony,nb", [(True, 24, 6), (False, 24, 6), (False, 256, 6), (False, 64, 26), (False, 2048, 6), (True, 2048, 6),
                                            (True, 24, 26), (False, 35, 6), (False, 36, 6)])
def test_memory_estimate_matches_the_allocator(ctx, lazy, colony, nb):
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("compares the estimate with the DEVICE's free memory, which other xdist workers change meanwhile: run without -n")
    n = 96
    free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=3, occ_prob=0.1)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    per_slot, per_field, fixed = api.memory_estimate(g, colony, 0, nb, lazy)
    # (2048 ants: the REF speculation buffers -- ~24 KB per ant, dense 6-neighbour solvers only -- and 2 GB of paths per slot)
    for slots in ((1, 2, 9, 17) if colony <= 256 else (1, 3)):
        ctx.sync()
        ctx.trim()       # (nothing kept: a kept block may serve a request up to a third smaller than itself as it stands, surplus included -- tests/test_gpu_arena.py)
        before, _ = ctx.memory_info()
        s = api.AcsSolver(ctx, g, n_slots=slots, max_colony=colony, neighbourhood=nb, lazy=lazy)
        ctx.sync()
        after, _ = ctx.memory_info()
        used = before - after
        pools = api.straggler_pool_bytes(g, slots, colony, 0, nb, lazy)
        assert (pools > 0) == (not lazy and slots <= 16 and colony <= 256)   # dense solvers of up to 16 slots and 256 ants hand their stragglers over, per slot
        want = slots * per_slot + (max(8, min(24, slots // 8)) if slots >= 32 else min(slots, 4)) * per_field + fixed + pools
        # the allocator rounds every block up (2 MiB granules): the estimate must not be below 90 % nor above 103 % of the truth.  (A solver is ~40
        # blocks, the small ones each rounded up to a granule: up to ~16 MiB the estimate does not count -- it only shows on a one-slot solver of this
        # size, and only in a process whose runtime has no freed small blocks to hand out again: this module run on its own.)
        assert 0.90 * used - (16 << 20) <= want <= 1.03 * used + (64 << 20), (slots, used, want)
        s.close()
    g.close()


def test_slot_rule_at_c5_shape(ctx):
    """256^3, 24 ants, 2 016 searches over 63 end points on ONE device: nine whole batches of 224 -- the measured optimum
     -- rather than 8 x 252 (past the footprint where the walk slows) or 224 x 9 with a remainder."""
    n = 256
    free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.1)
    g = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    fr, total = ctx.memory_info()
    if fr < 250e9:
        pytest.skip("less than 250 GB free on this device")
    slots, batches = api.pair_slots_by_rule(ctx, g, 24, 2016, 63, 150)
    assert (slots, batches) == (224, 9), (slots, batches)
    # 8 devices: 252 searches per shard fit one device's limit? no: two whole batches of 126
    assert api.pair_slots_by_rule(ctx, g, 24, 252, 8, 150) == (126, 2)
    # a small job is one batch
    assert api.pair_slots_by_rule(ctx, g, 24, 10, 4, 150) == (10, 1)
    g.close()
