"""Every refusal of the twelve voxel-search calls (geodesic, weighted, chamfer, chamfer_weighted, each as _fields, _matrix and _paths) on one
small grid: the return code, the exported function's own name in front of wa_last_error, and the keyword of the message.  The calls of a
family share their bodies and are handed their name, which is where a wrong one would slip in."""
import numpy as np
import pytest

from test_gpu_chamfer import grid_of
from welding_robot_amd import api

pytestmark = pytest.mark.gpu
ARG, CAPACITY = 1, 7
SENT = -77
P = lambda a: a.ctypes.data
LEAD = {"geodesic": (), "weighted": ("cost",), "chamfer": ("step",), "chamfer_weighted": ("step", "pen")}   # the arrays in front of the ids
CALLS = [(fam, kind) for fam in LEAD for kind in ("fields", "matrix", "paths")]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def test_every_refusal_names_its_call(ctx):
    dims = (9, 4, 3)
    free = np.ones(108, np.uint8)
    free[50] = 0
    g = grid_of(ctx, free, dims)
    lib = ctx.lib
    out = np.full(4 * 108, SENT, np.int32)
    lens = np.full(8, SENT, np.int32)
    ids_out = np.full(64, SENT, np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    step = lambda *v: np.array(v, np.int32)
    ok = dict(step=step(3, 4, 5), cost=np.full(108, 2, np.uint8), pen=np.full(108, 2, np.uint8), ids=i64(0, 107), ends=i64(107, 0),
              off=i64(0, 30, 60), ids_out=ids_out, out=out, lens=lens)
    ok["pen"][50] = 255   # (an occupied voxel's byte is ignored)
    ok["cost"][50] = 0

    def untouched():
        return (out == SENT).all() and (ids_out == SENT).all() and (lens == SENT).all()

    def keys(fam, kind):
        """the pointer arguments of a call, in its order"""
        tail = ("ids", "out") if kind != "paths" else ("ids", "ends", "off", "ids_out", "out") + (() if fam == "geodesic" else ("lens",))
        return LEAD[fam] + tail

    def call(fam, kind, cnt=2, **over):
        """(name, return code) of the call with the valid arguments, except those in `over` (an array, or None for NULL)"""
        a = dict(ok, **over)
        ptr = {k: None if a[k] is None else P(a[k]) for k in keys(fam, kind)}
        name = "wa_grid_%s_%s" % (fam, kind)
        if kind != "paths":
            args = [ptr[k] for k in LEAD[fam]] + [ptr["ids"], cnt, ptr["out"]]
        else:
            args = [ptr[k] for k in LEAD[fam]] + [ptr["ids"], ptr["ends"], cnt, ptr["off"], ptr["ids_out"], ptr["out"]] + ([] if fam == "geodesic" else [ptr["lens"]])
        return name, getattr(lib, name)(g.h, *args)

    def refused(fam, kind, code, keyword, **over):
        name, rc = call(fam, kind, **over)
        err = lib.wa_last_error(ctx.h)
        assert rc == code, (name, over.keys(), rc, err)
        assert err.startswith(name.encode() + b": "), (name, err)
        assert keyword in err, (name, err)

    cost_at = lambda v, c: np.where(np.arange(108) == v, c, ok["cost"]).astype(np.uint8)
    pen_at = lambda v, q: np.where(np.arange(108) == v, q, ok["pen"]).astype(np.uint8)
    checked = 0
    for fam, kind in CALLS:
        for k in keys(fam, kind):                                                       # NULL, one argument at a time
            refused(fam, kind, ARG, b"bad argument", **{k: None})
        refused(fam, kind, ARG, b"bad argument", cnt=-1)
        if "step" in LEAD[fam]:
            refused(fam, kind, ARG, b"step", step=step(0, 4, 5))
            refused(fam, kind, ARG, b"step", step=step(3, 4, 17))
        refused(fam, kind, ARG, b"outside the grid", ids=i64(0, 108))
        refused(fam, kind, ARG, b"occupied", ids=i64(0, 50))
        if kind == "paths":
            refused(fam, kind, ARG, b"outside the grid", ends=i64(-1, 0))
            refused(fam, kind, ARG, b"occupied", ends=i64(50, 0))
            refused(fam, kind, ARG, b"offsets decrease", off=i64(0, 30, 29))
        if fam == "weighted":
            refused(fam, kind, ARG, b"WA_COST_MAX", cost=cost_at(3, 0))
            refused(fam, kind, ARG, b"WA_COST_MAX", cost=cost_at(107, 9))
        if fam == "chamfer_weighted":
            refused(fam, kind, ARG, b"WA_PEN_MAX", pen=pen_at(49, 32))
        assert untouched(), (fam, kind)
        checked += 1
    assert checked == 12
    # a pair's range too short: the counts are written, the nodes of that pair are not
    for fam in LEAD:
        refused(fam, "paths", CAPACITY, b"shorter than its path", off=i64(0, 1, 31))
        assert ids_out[0] == SENT and ids_out[1] != SENT
        out[:] = SENT
        lens[:] = SENT
        ids_out[:] = SENT
    # a count of 0 returns before the penalties are looked at (here: an array that would be refused)
    for kind in ("fields", "matrix", "paths"):
        assert call("chamfer_weighted", kind, cnt=0, pen=np.full(108, 255, np.uint8))[1] == 0
    assert untouched()
    g.close()
