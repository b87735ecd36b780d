"""The host reads every window's verdict and does not enqueue the launches of committed generations (wa_acs_run, a lone search):
read-back on == WA_CONVERGED_READBACK=0 == the C oracle, bit for bit -- the five trace arrays, the best cost and path, the ants of the last
generation and the WHOLE pheromone field -- on the 12^3 searches of tests/test_gpu_converged_run.py (their generations that can be committed are
listed there).  The counters of wa_acs_converged_host_info are held against those of wa_acs_converged_info.  A committed window of j generations whose
verdict is read leaves out the launches of j - 2 of them: the first is enqueued behind the window while the host reads the verdict, the last is the
flush.  Behind a window that committed whole the next window's flush is enqueued speculatively, in place of its first generation, and a whole window
then leaves out j - 1 (WA_CONVERGED_SPECULATE=0 switches that off; every case runs both ways).  A window whose verdict is not read leaves out none, so

    generations - 2 * (whole + cut)  <=  generations not enqueued  <=  generations - (whole + cut).

Windows of fewer than three generations can leave nothing out and are not waited for."""
import os

import numpy as np
import pytest

import test_gpu_converged_run as R
from welding_robot_amd import api

pytestmark = pytest.mark.gpu

ctx = R.ctx          # (module-scoped fixtures of the cases' own module: one context, the grids made once)
dgrids = R.dgrids
KEYS = R.KEYS + ("WA_CONVERGED_READBACK", "WA_CONVERGED_WAIT_US", "WA_CONVERGED_SPECULATE")
ZERO = [0, 0, 0, 0]


def run(ctx, dgrids, case, env, pieces=None, profile=0, P=1, groups=1, stragglers=None, sync=True):
    """the search(es) of `case` with the switches in `env` (read when the solver is created).  Returns (results per slot, wa_acs_converged_info per
    slot, wa_acs_converged_host_info).  sync=False: the results are read straight behind the last run()."""
    n, occ, colony, rho, gens, seed = R.CASES[case]
    _, (sid, eid) = R.ogrid(n, occ)
    old = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        s = api.AcsSolver(ctx, dgrids(n, occ), n_slots=P, max_colony=colony)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    s.set_pipeline(groups)
    if stragglers is not None:
        s.set_stragglers(stragglers)
    p = api.default_params(max_iteration=gens, predict=float(colony / 0.35), fixed_colony=colony, rng_mode=api.RNG_DEV, seed=seed, rho=rho)
    s.begin(p, [sid] * P, [eid] * P, streams=list(range(P)))
    if profile:
        s.profile(True, profile)
    done = 0
    for c in (pieces or [gens]):
        c = min(c, gens - done)
        if c > 0:
            s.run(c)
            done += c
    if done < gens:
        s.run(gens - done)
    if sync:
        s.sync()
    out = [R.collect(s, q, gens) for q in range(P)]
    info = [s.converged_info(q) for q in range(P)]
    host = s.converged_host_info()
    s.close()
    return out, info, host


def three_way(ctx, dgrids, case, env, tag, **kw):
    """read-back on (with and without speculative flushes) == read-back off == oracle; the device's own counters do not depend on the read-back, and
    read-back off reports nothing.  Returns (wa_acs_converged_info of slot 0, wa_acs_converged_host_info with speculative flushes, ... without)."""
    on, info, host = run(ctx, dgrids, case, env, **kw)
    plain, info_plain, host_plain = run(ctx, dgrids, case, dict(env, WA_CONVERGED_SPECULATE=0), **kw)
    off, info_off, host_off = run(ctx, dgrids, case, dict(env, WA_CONVERGED_READBACK=0), **kw)
    print(tag, info[0], host, host_plain)
    for q in range(len(on)):
        want = R.ref(case, q)
        R.same(off[q], want, (tag, "off", q))
        R.same(plain[q], want, (tag, "on, no speculation", q))
        R.same(on[q], want, (tag, "on", q))
    assert info == info_off and info_plain == info_off, (tag, info, info_plain, info_off)
    assert host_off == ZERO, (tag, host_off)
    assert host_plain[2] == 0, (tag, host_plain)
    return info[0], host, host_plain


def bounds(info, host):
    committed, gens = info["whole"] + info["cut"], info["generations"]
    assert host[1] <= gens - committed, (info, host)
    assert host[1] >= gens - 2 * committed, (info, host)
    assert host[3] <= host[0] and host[2] <= host[0], host


@pytest.mark.parametrize("window", [1, 2, 3, 5, None])
def test_window_lengths(ctx, dgrids, window):
    """flushes of odd and even j, with and without generations left out in front of them"""
    env = {} if window is None else dict(WA_CONVERGED_WINDOW=window)
    info, host, plain = three_way(ctx, dgrids, "firm", env, ("window", window))
    assert info["generations"] > 0 and info["whole"] > 0, info
    bounds(info, host)
    bounds(info, plain)
    for h in (host, plain):
        if window in (3, 5, None):
            assert h[0] > 0 and h[1] > 0, h
        if window == 1:
            assert h[1] == 0, h


@pytest.mark.parametrize("window", [None, 3])
def test_cut_windows(ctx, dgrids, window):
    """0 < j < W: the flush sits in the middle of the window and full generations follow it.  The default window 64-95 is cut at generation 73 with no
    whole window in front; windows of 3 commit 66-68 and 69-71 whole (the second one's flush goes out speculatively) and 72-74 is cut at 73"""
    env = {} if window is None else dict(WA_CONVERGED_WINDOW=window)
    info, host, plain = three_way(ctx, dgrids, "partial", env, ("partial", window))
    assert info["cut"] > 0 and info["generations"] > 0, info
    bounds(info, host)
    bounds(info, plain)
    if window == 3:
        assert host[2] > 0, host       # a cut directly behind a whole window: its speculative flush was cancelled


def test_the_best_path_improves_after_committed_generations(ctx, dgrids):
    info, host, plain = three_way(ctx, dgrids, "improves", dict(WA_CONVERGED_WINDOW=1), "improves", pieces=[33], stragglers=0)
    assert info["generations"] > 0, info
    bounds(info, host)
    bounds(info, plain)
    assert host[1] == 0, host


def test_uneven_pieces(ctx, dgrids):
    """windows end with the call: every length from 1 on, waits at the end of short calls"""
    info, host, plain = three_way(ctx, dgrids, "firm", {}, "pieces", pieces=[1, 2, 7, 3, 11, 1, 1, 20, 5])
    assert info["generations"] > 0, info
    bounds(info, host)
    bounds(info, plain)


def test_profiling_with_period_3(ctx, dgrids):
    """windows of at most two generations between the stamped ones: nothing to leave out"""
    info, host, plain = three_way(ctx, dgrids, "firm", {}, "profile 3", profile=3)
    assert info["generations"] > 0, info
    bounds(info, host)
    bounds(info, plain)
    assert host[1] == 0, host


@pytest.mark.parametrize("case", ["small", "wide"])
def test_colony_against_the_block_count(ctx, dgrids, case):
    info, host, plain = three_way(ctx, dgrids, case, {}, ("colony", case))
    assert info["generations"] > 0, info
    bounds(info, host)
    bounds(info, plain)
    if case == "wide":
        assert host[1] > 0 and plain[1] > 0, (host, plain)


def test_best_path_longer_than_the_cap(ctx, dgrids):
    """every window leaves by its early way out (block 0 reports j = 0): verdicts are read, nothing is committed, nothing left out"""
    info, host, plain = three_way(ctx, dgrids, "firm", dict(WA_CONVERGED_NODES=16), "cap")
    assert info["enqueued"] > 0 and info["whole"] == info["cut"] == info["generations"] == 0, info
    assert host[0] > 0 and host[1] == 0, host
    bounds(info, host)
    bounds(info, plain)


def test_no_wait_at_all(ctx, dgrids):
    """WA_CONVERGED_WAIT_US=0: every wait is given up before the word is looked at, every generation is enqueued"""
    info, host, plain = three_way(ctx, dgrids, "firm", dict(WA_CONVERGED_WAIT_US=0), "wait 0")
    assert info["generations"] > 0, info
    for h in (host, plain):
        assert h[3] == h[0] > 0 and h[1] == 0 and h[2] == 0, h


@pytest.mark.parametrize("groups", [1, 2])
def test_batches_keep_their_enqueue(ctx, dgrids, groups):
    """three searches in one solver, on one stream and in two pipelined groups: no verdict is read"""
    info, host, plain = three_way(ctx, dgrids, "firm", {}, ("three", groups), P=3, groups=groups)
    assert info["generations"] > 0, info
    assert host == ZERO and plain == ZERO, (host, plain)


def test_results_read_without_a_sync(ctx, dgrids):
    info, host, plain = three_way(ctx, dgrids, "firm", {}, "no sync", sync=False)
    assert info["generations"] > 0 and host[1] > 0, (info, host)
    bounds(info, host)
    bounds(info, plain)
