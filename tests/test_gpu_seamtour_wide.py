"""wa_gtsp_seam_tour with more starts than the device holds at once, and at the largest jobs it accepts, against tests/seamtour_ref.py
byte for byte.

Several starts per team: st_launch caps the grid at the resident workgroups and every team loops `start += gridDim.x * TEAMS`, so with
n_starts = 2 * resident + 3 (resident: test_wide_input_rules.resident_starts for this device's compute units) every team descends a
second time and three teams a third -- on the swapped E / E2, the reused reduction words, behind the closing st_team_sync -- in each
storage case: a wavefront per descent with a 32-bit and with a 64-bit W, a workgroup per descent with W in LDS and in global memory.
A start's descent does not depend on the others, so a sample of starts is compared with seamtour_ref.random_start + descend, and every
start with what needs no descent.

Large M: M = 301, 513, 1024 and 1025 (move numbers up to 7 M^2 = 7.4 M, W indices up to 2050^2, a 64-bit W of 33 MB in global memory).
tests/test_wide_input_rules.py holds the jobs and checks on the CPU that their descents move."""
import concurrent.futures as cf
import ctypes as C
import multiprocessing as mp
import os

import numpy as np
import pytest

import seamtour_ref as R
import test_wide_input_rules as WR
from test_gpu_seamtour import same
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
WORKERS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


HIP_ATTR_MULTIPROCESSOR_COUNT = 63   # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)


@pytest.fixture(scope="module")
def compute_units(ctx):
    """what st_launch reads as ctx->prop.multiProcessorCount, asked of the HIP runtime the library itself is linked with"""
    v = C.c_int(0)
    assert ctx.lib.hipDeviceGetAttribute(C.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
    assert 1 <= v.value <= 4096
    if "MI355X" in str(ctx.device_name):
        assert v.value == 256, v.value          # (a guard against the attribute's number moving: the starts below are sized by it)
    return int(v.value)


@pytest.mark.parametrize("name", sorted(WR.MULTI))
def test_every_team_descends_more_than_once(ctx, compute_units, name):
    m, closed, _, max_passes, (team, w_lds, narrow) = WR.MULTI[name]
    M = m if closed else m + 1
    d, kw = WR.multi_job(name)
    resident = WR.resident_starts(M, narrow, compute_units)
    n_starts = WR.multi_starts(name, compute_units)
    assert n_starts == 2 * resident + 3 <= WR.MAX_STARTS
    # a sample of starts against their own descents, which worker processes compute while the device runs all of them
    sample = WR.sampled_starts(n_starts, resident)
    assert {0, 1, n_starts - 1, resident, 2 * resident - 1, 2 * resident} <= set(sample) and len(sample) >= 200
    with cf.ProcessPoolExecutor(WORKERS, mp_context=mp.get_context("spawn")) as pool:
        jobs = pool.map(WR.descents, [(name, sample[i::WORKERS]) for i in range(WORKERS)])
        got = api.seam_tour(ctx, d, n_starts=n_starts, **kw)
        want = sorted(r for part in jobs for r in part)
    W = R.quantise(d, m, closed)
    assert bool((W >> 32).any()) != narrow and WR.seam_storage(M, narrow)[:2] == (team, w_lds)
    cost, passes, s = got["start_cost_q"], got["start_passes"], got["summary"]
    assert [w[0] for w in want] == sample
    capped = 0
    for r, c_q, p, c in want:
        assert (int(cost[r]), int(passes[r])) == (c_q, p), (name, r, int(cost[r]), int(passes[r]), c_q, p)
        capped += c
    # every start: what needs no descent
    assert cost.dtype == np.int64 and passes.dtype == np.int32 and len(cost) == len(passes) == n_starts
    assert got["cost_q"] == s["cost_q"] == int(cost.min()) and s["best_start"] == int(np.argmin(cost))      # (argmin: the first minimum)
    assert s["passes_total"] == int(passes.astype(np.int64).sum()) and s["n_starts"] == n_starts and (s["m"], s["M"]) == (m, M)
    assert (passes >= 1).all() and (passes <= max_passes).all()
    if max_passes == 3:
        assert capped == len(sample) and s["n_capped"] == int((passes == 3).sum()) == n_starts   # (a start at the cap that had converged would not count)
    else:
        assert capped == 0 and s["n_capped"] == 0
    assert s["start0_cost_q_out"] == int(cost[0]) and s["start0_cost_q_in"] == R.tour_cost(R.start0(m, closed), W) >= int(cost[0])
    assert sorted(got["order"].tolist()) == list(range(m)) and set(got["dir"].tolist()) <= {0, 1}
    E = R.start0(m, closed, got["order"], got["dir"])
    assert R.tour_cost(E, W) == got["cost_q"]                            # the returned order, re-costed
    if name == "wave_narrow":
        exact = R.seam_tour_exact(d, m, closed)["cost_q"]
        assert (cost >= exact).all()
    print(name, "compute units", compute_units, "resident", resident, "starts", n_starts, "sampled", len(sample), "passes", int(passes.min()), "..",
          int(passes.max()), "distinct costs", len(set(cost.tolist())))


@pytest.mark.parametrize("name", sorted(WR.LARGE))
def test_large_jobs_are_bit_equal_to_the_restatement(ctx, name):
    m, closed, scale = WR.LARGE[name]
    d, kw = WR.large_job(name)
    want = R.seam_tour(d, m, **kw)
    got = api.seam_tour(ctx, d, **kw)
    same(got, want)
    assert want["summary"]["n_capped"] == 2 and want["start_passes"].tolist() == [3, 3]
    assert got["cost_q"] < want["summary"]["start0_cost_q_in"]
