"""GPU tests of what the trajectory stages share: the lookup view of a grid (its distance field, and the range and monotonicity of its
axis tables, computed once per grid by whichever call needs them first) and the clearance summary.  All on clearance_ref's shuffled
scene: a stretched x table, a shuffled y table and a repeated last z node."""
import numpy as np
import pytest

import clearance_ref as CR
import retime_ref as R
import torch_ref as T
from welding_robot_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _clearance_same(t, g, free, axes, xyz):
    out = t.clearance(g)
    want = CR.clearance(free, g.distance_field(), g.nx, g.ny, g.nz, axes[0], axes[1], axes[2], xyz)
    for got, w in zip(out[:3], want[:3]):
        assert np.array_equal(got, w)
    assert out[3] == want[3], (out[3], want[3])
    return out


@pytest.mark.parametrize("retime_first_on", [0, 1])
def test_the_view_belongs_to_its_grid_whoever_builds_it(ctx, retime_first_on):
    """two grids of one context, same occupancy and dims, different tables.  On fresh grids the first call is a retime on one and a
    tool check on the other -- no clearance call has run on either -- then clearance on both in turn: every result equals its
    restatement, and the third call's arrays are the first call's"""
    free, dims, shuffled, xyz = CR.shuffled_scene()
    axes = [shuffled, R.unit_axes(dims)]
    grids = [api.Grid.from_occupancy(ctx, free, a[0], a[1], a[2], 1.0, 0) for a in axes]
    refs = [R.make_grid(free, dims, a) for a in axes]
    t = api.Trajectory.from_points(ctx, xyz)
    a, b = retime_first_on, 1 - retime_first_on

    lim = R.limits(v_max=2, acc=4, dec=4, v_near=0.25, near_d2=2)
    want = R.retime(xyz, lim, None, refs[a], 0.01)
    time_q, w_q, bound, ticks, s = t.retime(lim["v_max"], lim["acc"], lim["dec"], 0.01, a_lat=lim["a_lat"], grid=grids[a],
                                            v_near=lim["v_near"], near_d2=lim["near_d2"])
    assert s == want["summary"], (s, want["summary"])
    assert np.array_equal(time_q, want["time_q"]) and np.array_equal(w_q, want["w_q"]) and np.array_equal(bound, want["bound"])
    assert ticks.points().tobytes() == np.ascontiguousarray(want["ticks"], np.float32).tobytes()

    rs = np.random.RandomState(3)
    tool_axes = rs.normal(size=(len(xyz), 3)).astype(np.float32)
    tool = T.rod(5, 16 * 4, 1)
    cb, cn, cs = T.check(refs[b], xyz, tool_axes, tool, 4)
    blocked, near, s = t.torch_check(grids[b], tool_axes, tool, 4)
    assert np.array_equal(blocked, cb) and np.array_equal(near, cn) and s == cs, (s, cs)

    first = _clearance_same(t, grids[0], free, axes[0], xyz)
    second = _clearance_same(t, grids[1], free, axes[1], xyz)
    third = _clearance_same(t, grids[0], free, axes[0], xyz)
    for x, y in zip(first[:3], third[:3]):
        assert x.tobytes() == y.tobytes()
    assert first[3] == third[3]
    assert first[3]["n_outside"] > 0 and not np.array_equal(first[0], second[0])   # the tables matter: the grids answer differently
    for o in (ticks, t, grids[0], grids[1]):
        o.close()


def test_the_fit_reports_the_summary_of_its_samples(ctx):
    """wa_grid_fit_trajectory's `final` is the clearance summary of the samples it returns, field by field, on a grid with shuffled tables"""
    free, dims, axes, _ = CR.shuffled_scene()
    g = api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)
    poly = api.Trajectory.from_points(ctx, np.array([[-0.5, 0.5, 0.5], [2.0, 6.5, 3.0], [4.2, 1.0, 8.5], [0.5, 7.5, 9.5]], np.float32))
    b, samples, _, s = poly.fit(g, 3, 0.5, 6, 257)
    assert len(samples) == 257
    want = samples.clearance(g)[3]
    assert set(s["final"]) == set(want)
    for k in want:
        assert s["final"][k] == want[k], (k, s["final"], want)
    for o in (samples, b, poly, g):
        o.close()
