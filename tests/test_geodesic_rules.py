"""CPU checks of the exact shortest-path fields (wa_grid_geodesic_fields / _matrix / _paths): the header declares them and the library
exports them with the ctypes signatures, each refuses a NULL grid, and the numpy restatement the GPU tests compare against
(tests/geodesic_ref.py) gives hand-made answers and agrees with two independent checks (scipy.ndimage.label for reachability, a plain
queue for hop counts) on seeded random grids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geodesic_ref as G
from welding_robot_amd import _lib as L
from welding_robot_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_V, _P, _I = C.c_void_p, C.c_void_p, C.c_int32
DECLS = {
    "wa_grid_geodesic_fields": (["const wa_grid *g", "const int64_t *src_ids", "int32_t n_src", "int32_t *hops_out"], [_V, _P, _I, _P]),
    "wa_grid_geodesic_matrix": (["const wa_grid *g", "const int64_t *point_ids", "int32_t n_pts", "int32_t *hops_out"], [_V, _P, _I, _P]),
    "wa_grid_geodesic_paths": (["const wa_grid *g", "const int64_t *start_ids", "const int64_t *end_ids", "int32_t n_pairs",
                                "const int64_t *off", "int64_t *ids_out", "int32_t *hops_out"], [_V, _P, _P, _I, _P, _P, _P]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_and_library_exports(lib, name):
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, name + " is not declared"
    want, args = DECLS[name]
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == want
    assert hasattr(lib, name)
    res, sym_args = L.SYMBOLS[name]
    assert res is C.c_int and sym_args == args
    assert getattr(lib, name).argtypes == args


def test_hops_none_is_minus_one():
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    assert re.search(r"#define\s+WA_HOPS_NONE\s+\(-1\)", hdr) and L.WA_HOPS_NONE == -1 == G.NONE


def test_null_grid_is_refused(lib):
    ids, off = np.zeros(2, np.int64), np.array([0, 2], np.int64)
    hops, out = np.zeros(4, np.int32), np.zeros(2, np.int64)
    assert lib.wa_grid_geodesic_fields(None, ids.ctypes.data, 1, hops.ctypes.data) == 1
    assert lib.wa_grid_geodesic_matrix(None, ids.ctypes.data, 2, hops.ctypes.data) == 1
    assert lib.wa_grid_geodesic_paths(None, ids.ctypes.data, ids.ctypes.data, 1, off.ctypes.data, out.ctypes.data, hops.ctypes.data) == 1
    assert not hops.any() and not out.any()


@pytest.mark.parametrize("case", G.hand_cases(), ids=lambda c: c[0])
def test_restatement_hand_cases(case):
    name, free, dims, src, want = case
    h = G.field(free, dims, src)
    assert h.dtype == np.int32 and h[src] == 0
    for v, k in want.items():
        assert h[v] == k, (name, v, int(h[v]), k)
    assert ((h == G.NONE) | (free != 0)).all(), "an occupied voxel has no hop count"


def test_restatement_tie_is_decided_by_the_neighbour_order():
    free, dims, s, e, want = G.tie_case()
    hops, paths = G.paths(free, dims, [s, e, s], [e, s, s])
    assert hops.tolist() == [3, 3, 0]
    assert paths[0].tolist() == want
    # the rule is applied walking back from the END: the reverse pair is not the reversed path
    assert paths[1].tolist() == [7, 3, 1, 0]
    assert paths[2].tolist() == [0]
    for p, (a, b) in zip(paths, ((s, e), (e, s), (s, s))):
        G.check_path(free, dims, p, a, b, len(p) - 1)


def test_restatement_unreachable_pair_has_no_path():
    name, free, dims, src, want = G.hand_cases()[3]
    hops, paths = G.paths(free, dims, [src, 12], [12, 12])
    assert hops.tolist() == [G.NONE, 0] and paths[0] is None and paths[1].tolist() == [12]


def test_serpentine_and_baffles_are_what_they_say():
    f = G.serpentine(7, 5)
    h = G.field(f, (7, 5, 1), 0)
    assert int(f.sum()) == 3 * 7 + 2 and h.max() == int(f.sum()) - 1 and h[4 * 7 + 6] == h.max()
    f = G.baffles(12, 3, 3)   # walls at x = 2, 5, 8 with gaps at (y, z) = (0, 0), (2, 2), (0, 0)
    h = G.field(f, (12, 3, 3), 0)
    assert h[11] == 11 + 4 + 4 and (h[f != 0] >= 0).all()


@pytest.mark.parametrize("seed", range(36))
def test_restatement_against_label_and_queue(seed):
    from scipy import ndimage
    rs = np.random.RandomState(1000 + seed)
    dims = tuple(int(v) for v in rs.randint(1, 9, 3))
    if seed % 6 == 0:
        dims = (int(rs.randint(60, 70)), dims[1], dims[2])
    occ = (0.1, 0.3, 0.45)[seed % 3]
    n = int(np.prod(dims))
    free = (rs.uniform(size=n) >= occ).astype(np.uint8)
    src = int(rs.randint(n))
    free[src] = 1
    h = G.field(free, dims, src)
    lab, _ = ndimage.label(free.reshape(dims[2], dims[1], dims[0]) != 0)   # (the default structure is the 6-neighbourhood)
    lab = lab.reshape(-1)
    assert np.array_equal(h >= 0, lab == lab[src])
    assert np.array_equal(h, G.queue_field(free, dims, src))
    ends = rs.randint(n, size=4)
    for e in ends[free[ends] != 0]:
        p = G.walk_back(h, dims, int(e))
        if h[e] < 0:
            assert p is None
        else:
            G.check_path(free, dims, p, src, int(e), int(h[e]))


def test_bellman_check_refuses_wrong_fields():
    """geodesic_ref.bellman_exact, the whole-field checker of the 2^27-voxel GPU test: it accepts the true field and refuses fields that
    are off by one or two somewhere, that miss a reachable voxel, or that count an enclosed pocket"""
    dims = (9, 8, 7)
    n = 9 * 8 * 7
    free = (np.random.RandomState(3).uniform(size=n) >= 0.3).astype(np.uint8)
    src, pocket = 0, 4 + 9 * (4 + 8 * 3)
    free[src] = free[pocket] = 1
    for v in G.neighbours(pocket, dims):
        free[v] = 0
    h = G.field(free, dims, src)
    assert h.max() > 10 and (h >= 0).sum() > 250 and h[pocket] == G.NONE, "the source must see most of the box for the cases below to mean anything"
    for slab in (1, 3, 32):
        assert G.bellman_exact(h, free, dims, src, slab=slab)
    far = int(np.argmax(h))
    for v, d in ((far, 1), (far, -1), (int(np.flatnonzero(h == 3)[0]), 2)):
        w = h.copy()
        w[v] += d
        assert not G.bellman_exact(w, free, dims, src, slab=3)
    w = h.copy()
    w[far] = G.NONE
    assert not G.bellman_exact(w, free, dims, src, slab=3)
    w = h.copy()
    w[pocket] = 5
    assert not G.bellman_exact(w, free, dims, src, slab=3)
