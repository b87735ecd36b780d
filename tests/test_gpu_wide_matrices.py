"""GPU tests of the six distance-matrix calls with more points than the 256 threads of the block that looks the targets up
(geo_lookup_targets / pose_lookup_targets: the second and third trip of `t += 256`, the vote of threads that took different numbers of
trips, stop[s] set with the targets of a row spread over several trips), and of wa_grid_geodesic_fields with more sources than one
launch's gridDim.y.  Expected values are the `*_fields` restatements indexed at the points, as test_gpu_geodesic.test_baffles takes
them; every comparison is np.array_equal on int32.  tests/test_wide_input_rules.py holds the scene and the point lists and checks what
they decide."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import chamfer_ref as C
import chamfer_weighted_ref as CW
import geodesic_ref as G
import pose_ref as PR
import pose_weighted_ref as PW
import test_wide_input_rules as WR
import weighted_ref as W
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("geodesic", "weighted", "chamfer", "chamfer_weighted", "pose", "pose_weighted")
STEP = (3, 4, 5)
POSE_TABLE = dict(hop=2, turn_costs=[0, 1, 4])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def grid_of(ctx, grid):
    free, _, _, axes = grid
    return api.Grid.from_occupancy(ctx, free, axes[0], axes[1], axes[2], 1.0, 0)


def scene_costs(c):
    """what the weighted calls charge on the scene: (entry costs 1 .. 4 from the clearance, penalties 0 .. 3, pose bands)"""
    free, d2 = c["grid"][0], c["grid"][1]
    cost = W.clearance_costs(free, d2, [1, 4, 9])
    pen = WR.near_pen(c["grid"])
    return cost, pen, PW.bands_for(c["dirs"], WR.MATRIX_TURN, 2)


def device_matrix(g, c, call, pts, pins):
    cost, pen, bands = scene_costs(c)
    if call == "geodesic":
        return g.geodesic_matrix(pts)
    if call == "weighted":
        return g.weighted_matrix(cost, pts)
    if call == "chamfer":
        return g.chamfer_matrix(STEP, pts)
    if call == "chamfer_weighted":
        return g.chamfer_weighted_matrix(STEP, pen, pts)
    if call == "pose":
        return g.pose_matrix(c["dirs"], c["tool"], WR.MATRIX_TURN, pts, pins)
    return g.pose_weighted_matrix(c["dirs"], c["tool"], WR.MATRIX_TURN, api.pose_costs(POSE_TABLE["hop"], bands, POSE_TABLE["turn_costs"], pen), pts, pins)


_ROWS = {}      # (call, source key) -> what the restatement's field of that source gives a target: shared by every list, never modified
_SCENES = {}


def expected_matrix(c, call, pts, pins):
    """the rows of the restatement's fields indexed at the points (and, for the pose calls, at the targets' pins)"""
    free, dims = c["free"], c["dims"]
    cost, pen, bands = scene_costs(c)
    pts = np.asarray(pts, np.int64)
    posed = call.startswith("pose")
    if posed and call not in _SCENES:
        base = PR.Scene(c["grid"], c["dirs"], c["tool"], WR.MATRIX_TURN, c["opened"])
        _SCENES[call] = base if call == "pose" else PW.Scene(c["grid"], c["dirs"], c["tool"], WR.MATRIX_TURN,
                                                             PW.Costs(POSE_TABLE["hop"], bands, POSE_TABLE["turn_costs"], pen), base)
    out = np.empty((len(pts), len(pts)), np.int32)
    for i, s in enumerate(pts.tolist()):
        key = (call, s, int(pins[i]) if posed else -1)
        if key not in _ROWS:
            if call == "geodesic":
                _ROWS[key] = G.field(free, dims, s)
            elif call == "weighted":
                _ROWS[key] = W.field(free, cost, dims, s)
            elif call == "chamfer":
                _ROWS[key] = C.field(free, STEP, dims, s)
            elif call == "chamfer_weighted":
                _ROWS[key] = CW.field(free, STEP, pen, dims, s)
            else:
                _ROWS[key] = _SCENES[call].levels(s, int(pins[i]))      # (state [K, n], least over the directions [n])
        f = _ROWS[key]
        if posed:
            state, least = f
            out[i] = np.where(pins < 0, least[pts], state[np.maximum(pins, 0), pts])
        else:
            out[i] = f[pts]
    return out


@pytest.mark.parametrize("P", WR.MATRIX_SIZES + (WR.OPEN_SIZE,))
@pytest.mark.parametrize("call", CALLS)
def test_matrix_of_more_points_than_a_block_has_threads(ctx, call, P):
    c = WR.matrix_case()
    pts, pins = c["lists"][P]
    g = grid_of(ctx, c["grid"])
    got = device_matrix(g, c, call, pts, pins)
    g.close()
    want = expected_matrix(c, call, pts, pins)
    assert got.dtype == np.int32 and got.shape == (P, P)
    assert np.array_equal(got, want), (call, P, np.argwhere(got != want)[:8])
    if P == WR.OPEN_SIZE:
        assert (want >= 0).all()                                         # every row completes: stop[s] is set for every source
    else:
        assert (want == -1).any() and (want > 0).any()
    if P != WR.OPEN_SIZE:
        assert (want[:, 256:] == -1).any() and (want[:, 256:] > 0).any() and (want[256:, :256] > 0).any()


CHILD = """import sys; sys.path[:0] = [%r, %r]
import test_wide_input_rules as WR
from welding_robot_amd import api
from test_gpu_wide_matrices import CALLS, device_matrix, digest, grid_of
c = WR.matrix_case(); x = api.Context(0); g = grid_of(x, c['grid'])
pts, pins = c['lists'][257]
print('digest', *[digest(device_matrix(g, c, call, pts, pins)) for call in CALLS])
"""


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


@pytest.fixture(scope="module")
def one_source_per_chunk():
    """the digests of the six 257-point matrices computed one source per chunk (WA_GEO_CHUNK=1) in a fresh child process"""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, WA_GEO_CHUNK="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1].split()
    return dict(zip(CALLS, line[1:]))


@pytest.mark.parametrize("call", CALLS)
def test_chunking_does_not_change_the_rows(ctx, one_source_per_chunk, call):
    c = WR.matrix_case()
    pts, pins = c["lists"][257]
    g = grid_of(ctx, c["grid"])
    whole = device_matrix(g, c, call, pts, pins)
    g.close()
    assert one_source_per_chunk[call] == digest(whole)


def test_more_sources_than_one_launch(ctx):
    """65 535 + 70 sources on 3 x 2 x 2: the chunk loop's natural split at WA_GEO_MAX_CHUNK, the second chunk's rows land behind the
    first's"""
    free, src = WR.many_sources()
    ax = lambda n: np.arange(n, dtype=np.float32)   # noqa: E731
    g = api.Grid.from_occupancy(ctx, free, ax(3), ax(2), ax(2), 1.0, 0)
    got = g.geodesic_fields(src)
    g.close()
    assert got.shape == (WR.MAX_CHUNK + WR.MANY_EXTRA, 12) and got.dtype == np.int32
    rows = {int(s): G.field(free, WR.MANY_DIMS, int(s)) for s in np.unique(src)}
    want = np.stack([rows[int(s)] for s in src])
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]
    for s, row in WR.MANY_BY_HAND.items():
        assert got[s].tolist() == row, s
