"""The tool frames and the weld weave at jerk-limited ticks at the product boundary: the header declares the call, the library exports
it, the bindings match the header's structs, NULL arguments are answered with WA_ERR_ARG, the Python wrapper and weave_pattern exist
and examples/weave_demo.py runs.  Only the last test needs a device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import frames_ref as F
from welding_robot_amd import _lib as L
from welding_robot_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1
CALL = "wa_traj_retime_jerk_frames"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


def header_code():
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_and_library_exports_the_call(lib):
    code = header_code()
    assert re.search(r"\bint\s+%s\s*\(" % CALL, code) and CALL in L.SYMBOLS and hasattr(lib, CALL)
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % CALL, code, flags=re.S).group(1)
    assert len(proto.split(",")) == len(L.SYMBOLS[CALL][1]) == len(L.SYMBOLS["wa_traj_retime_jerk_axes"][1]) + 3   # weave, lat_out, frames
    assert "const wa_weave *weave" in proto and "wa_traj **lat_out" in proto and "wa_frames_summary *frames" in proto
    rest = [a for a in L.SYMBOLS[CALL][1] if a not in (C.POINTER(L.Weave), C.POINTER(L.FramesSummary))]
    axes = list(L.SYMBOLS["wa_traj_retime_jerk_axes"][1])
    assert rest[:len(axes) - 4] + rest[len(axes) - 3:] == axes   # (lat_out sits behind blocked_out, in front of the summaries)


def test_both_structs_match_the_bindings():
    code = header_code()
    body = code.split("wa_frames_summary;")[0].rsplit("typedef struct", 1)[1]
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, _ in L.FramesSummary._fields_] == list(F.FRAMES_FIELDS)
    assert C.sizeof(L.FramesSummary) == 64 and all(t is C.c_int64 for _, t in L.FramesSummary._fields_)
    body = code.split("wa_weave;")[0].rsplit("typedef struct", 1)[1]
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, _ in L.Weave._fields_]
    assert [t for _, t in L.Weave._fields_] == [C.c_double] * 3 + [C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8]
    assert (L.Weave.pattern.offset, L.Weave.P.offset, L.Weave.tag_mask.offset, L.Weave.tag_value.offset, C.sizeof(L.Weave)) == (24, 32, 36, 37, 40)
    assert "const int16_t *pattern" in body


def test_the_header_numbers_the_rules(lib):
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    section = hdr.split("tool frames and the weld weave at jerk-limited ticks")[1]
    for k in range(61, 68):
        assert re.search(r"^ \* %d\. " % k, section, flags=re.M), k
    assert "1 .. 2^50" in section   # (the range of wl_q is settled in the rule)


def test_null_arguments_are_answered_not_followed(lib):
    assert getattr(lib, CALL)(*[0.01 if a is C.c_double else (4 if a is C.c_int32 else None) for a in L.SYMBOLS[CALL][1]]) == ARG


def test_the_python_wrapper_and_the_patterns_exist():
    assert callable(api.Trajectory.retime_jerk_frames) and callable(api.make_weave)
    for kind in ("triangle", "sine", "trapezoid"):
        for P in (2, 3, 16, 4096):
            p = api.weave_pattern(kind, P)
            assert p.dtype == np.int16 and p.shape == (P,) and p[0] == 0 and np.abs(p.astype(np.int64)).max() <= 16384
        p = api.weave_pattern(kind, 64).astype(np.int64)
        assert p[16] == 16384 and p[48] == -16384 and p[32] == 0 and np.array_equal(p[1:], -p[:0:-1])   # (odd about the half period)
    assert np.array_equal(api.weave_pattern("triangle", 16), F.triangle(16))
    assert (np.abs(api.weave_pattern("trapezoid", 64)[8:25]) == 16384).all()
    for bad in (("triangle", 1), ("triangle", 4097), ("square", 8)):
        with pytest.raises(ValueError):
            api.weave_pattern(*bad)
    w = api.make_weave(0.5, 2.0, api.weave_pattern("sine", 32), taper=0.25, tag_mask=3, tag_value=1)
    assert (w.amplitude, w.wavelength, w.taper, w.P, w.tag_mask, w.tag_value) == (0.5, 2.0, 0.25, 32, 3, 1) and w.pattern


@pytest.mark.gpu
def test_the_weave_demo_runs():
    """approach, stop, one woven pass, stop, retreat in a two-plate corner of 32^3 voxels"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "weave_demo.py"), "--grid", "32"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    f, a = out["frames"], out["axes"]
    assert f["n_ticks"] == a["n_ticks"] == out["jerk"]["n_ticks"] > out["jerk"]["window"] and f["n_weave_runs"] == 1
    assert 0 < f["n_weave_ticks"] < f["n_ticks"] and f["n_no_lateral"] == 0 and f["n_weave_blocked"] == 0 and a["n_blocked"] == 0
    assert 0 < f["max_offset_q"] <= round(out["weave"]["amplitude"] * 2 ** 30) and out["stops"]["n_stops"] == 2
    assert out["plain"]["max_offset_q"] == 0 and out["plain"]["n_weave_ticks"] == 0 and out["moved_ticks"] > 0
