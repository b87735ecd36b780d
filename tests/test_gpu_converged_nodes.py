"""The window kernel's dealing of the best path's nodes over its blocks (k_converged_run, csrc/acs_converged.hpp; WA_CONVERGED_BLOCKS = B, read when
the solver is created): block b owns nodes [b m, (b + 1) m), m = ceil(best_len / B), advances them and checks every ant of the colony at them.

The searches are the 12^3 ones of test_gpu_converged_run.py (its docstring lists the generations the oracle says can be committed); their converged
best path has 22 nodes, so B = 1 puts all nodes into one block (several advance trips per wavefront), 3 gives shares of 8, 8, 6, 7 gives 4 and a last
share of 2, 22 one node each, 32 and the default leave blocks without nodes.  Every case is the three-way comparison of that module, bit for bit:
mechanism on == WA_CONVERGED_RUN=0 == the C oracle in DEV mode, over the five trace arrays, the best cost and path, the ants of the last generation
and the whole pheromone field; and every case asserts from wa_acs_converged_info that generations were committed.  The run with the mechanism off
does not depend on B: it is made once per search and shared."""
import contextlib
import os

import pytest

import test_gpu_converged_run as R
from test_gpu_converged_run import ctx, dgrids  # noqa: F401  (the module-scoped context and device grids)

pytestmark = pytest.mark.gpu

BLOCKS = [1, 3, 7, 22, 32, None]   # None: the default
_off = {}


@contextlib.contextmanager
def blocks(b):
    old = os.environ.get("WA_CONVERGED_BLOCKS")
    try:
        os.environ.pop("WA_CONVERGED_BLOCKS", None)
        if b is not None:
            os.environ["WA_CONVERGED_BLOCKS"] = str(b)
        yield
    finally:
        os.environ.pop("WA_CONVERGED_BLOCKS", None)
        if old is not None:
            os.environ["WA_CONVERGED_BLOCKS"] = old


def three_way(ctx, dgrids, case, b, env=None, **kw):
    """mechanism on with B = b == mechanism off == oracle; returns the counters per slot of the run with the mechanism on"""
    env = dict(env or {})
    key = (case, tuple(sorted(env.items())), tuple(sorted(kw.items())))
    if key not in _off:
        off, info_off = R.gpu(ctx, dgrids, case, dict(env, WA_CONVERGED_RUN=0), **kw)
        for q in range(len(off)):
            R.same(off[q], R.ref(case, q), (case, "off", q))
            assert info_off[q] == dict(enqueued=0, whole=0, cut=0, generations=0), (case, q, info_off[q])
        _off[key] = off
    with blocks(b):
        on, info = R.gpu(ctx, dgrids, case, env, **kw)
    for q in range(len(on)):
        R.same(on[q], R.ref(case, q), (case, b, "on", q))
        R.same(on[q], _off[key][q], (case, b, "on == off", q))
    return info


@pytest.mark.parametrize("b", BLOCKS)
def test_dealings(ctx, dgrids, b):
    """all nodes in one block / shares 8, 8, 6 / 4 and a last share of 2 / one node each / blocks without nodes"""
    info = three_way(ctx, dgrids, "firm", b)[0]
    assert info["generations"] > 0 and info["whole"] > 0, info


@pytest.mark.parametrize("b", BLOCKS)
def test_dealings_with_windows_cut_by_a_deviating_ant(ctx, dgrids, b):
    """rho 0.9: the node at which an ant leaves the path falls into a different block with every dealing; the smallest t over the blocks decides j"""
    info = three_way(ctx, dgrids, "partial", b)[0]
    assert info["cut"] > 0 and info["generations"] > 0, info


@pytest.mark.parametrize("case", ["wide", "small"])
def test_colony_against_the_checking_lanes(ctx, dgrids, case):
    """64 ants: exactly one wavefront of checking lanes; 20 ants: well short of one"""
    info = three_way(ctx, dgrids, case, 3)[0]
    assert info["generations"] > 0, info


@pytest.mark.parametrize("window", [1, 2, 5])
def test_window_lengths_over_three_blocks(ctx, dgrids, window):
    """odd and even j; the flush reads snapshot j - 1, which three blocks wrote their shares of"""
    info = three_way(ctx, dgrids, "firm", 3, dict(WA_CONVERGED_WINDOW=window))[0]
    assert info["generations"] > 0 and info["whole"] > 0, info


@pytest.mark.parametrize("groups", [1, 2])
def test_three_searches_in_one_solver(ctx, dgrids, groups):
    """the ticket and the smallest t are per slot; streams 0, 1, 2 settle at different generations"""
    info = three_way(ctx, dgrids, "firm", 7, P=3, groups=groups)
    assert all(i["generations"] > 0 for i in info), info
    assert len({i["generations"] for i in info}) > 1, info


def test_block_counts_out_of_range_are_clamped(ctx, dgrids):
    """0 -> 1 block, 100 000 -> 256 blocks: the same results (each equal to the oracle's) and the same counters"""
    low = three_way(ctx, dgrids, "firm", 0)[0]
    high = three_way(ctx, dgrids, "firm", 100000)[0]
    assert low == high and low["generations"] > 0 and low["whole"] > 0, (low, high)
