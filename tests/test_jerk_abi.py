"""The jerk-limited ticks at the product boundary, without a device: the header declares the two calls, the library exports them, the
binding matches the header's struct, the calls answer NULL arguments with WA_ERR_ARG, the helper computes the window, the Python
wrappers exist and examples/plan_batch.py knows --jerk."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import jerk_ref as J
from welding_robot_amd import _lib as L
from welding_robot_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1
CALLS = ("wa_traj_retime_jerk", "wa_traj_jerk_window")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


def header_code():
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def struct_fields(code, name):
    body = code.split(name + ";")[0].rsplit("typedef struct", 1)[1]
    return re.findall(r"\b(\w+)\s*[,;]", body)


def test_header_declares_and_library_exports_the_calls(lib):
    code = header_code()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(L.SYMBOLS[name][1]), name
    assert struct_fields(code, "wa_jerk_summary") == [f for f, _ in L.JerkSummary._fields_] == list(J.JERK_FIELDS)
    assert C.sizeof(L.JerkSummary) == 96 and all(t is C.c_int64 for _, t in L.JerkSummary._fields_)
    assert len(L.SYMBOLS["wa_traj_retime_jerk"][1]) == len(L.SYMBOLS["wa_traj_retime_stops"][1]) + 5   # window, seg_tag, s_q, tag, jerk


def test_null_arguments_are_answered_not_followed(lib):
    assert lib.wa_traj_retime_jerk(None, None, None, None, None, 0.01, 4, None, None, None, None, None, None, None, None, None, None) == ARG
    assert lib.wa_traj_jerk_window(None, 1.0, 1.0, 1.0, 0.001, None) == ARG


def test_the_window_helper(lib):
    w = C.c_int32(-5)
    for acc, dec, jerk, tick in ((2.0, 4.0, 1000.0, 0.001), (1.0, 1.0, 1e9, 1.0), (3.0, 1.0, 7.0, 0.004), (1.0, 1.0, 2.0, 2.0 ** -20)):
        assert lib.wa_traj_jerk_window(None, acc, dec, jerk, tick, C.byref(w)) == 0
        assert w.value == J.jerk_window(acc, dec, jerk, tick) == api.jerk_window(acc, dec, jerk, tick)
    w.value = -5
    for bad in ((0.0, 1, 1, 1), (1, -1.0, 1, 1), (1, 1, float("inf"), 1), (1, 1, 1, float("nan")), (1e9, 1, 1e-9, 1e-9), (1, 1, 1, 2.0 ** -21)):
        assert lib.wa_traj_jerk_window(None, *[float(x) for x in bad], C.byref(w)) == ARG and w.value == -5, bad
        with pytest.raises(ValueError):
            api.jerk_window(*bad)


def test_python_wrappers_exist():
    assert callable(api.Trajectory.retime_jerk) and callable(api.jerk_window)


def test_plan_batch_refuses_jerk_where_it_does_not_apply():
    exe = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py")]
    r = subprocess.run(exe + ["--jerk", "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--retime" in r.stderr and "--weld-passes" in r.stderr, r.stderr[-300:]
    r = subprocess.run(exe + ["--retime", "--torch", "8", "--tick-poses", "1.0", "--jerk", "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--tick-poses" in r.stderr, r.stderr[-300:]
    r = subprocess.run(exe + ["--seams", "--jerk", "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr[-300:]
