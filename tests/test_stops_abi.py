"""The weld-pass stage at the product boundary, without a device: the header declares the three calls, the library exports them, the
bindings match the header's structs, the calls answer NULL arguments with WA_ERR_ARG, the Python wrappers exist and
examples/plan_batch.py knows --weld-passes."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from welding_robot_amd import _lib as L
from welding_robot_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1
CALLS = ("wa_traj_retime_stops", "wa_traj_tick_axes_stops", "wa_traj_axes_dwells")


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
    for cname, struct, size in (("wa_stops_summary", L.StopsSummary, 24), ("wa_tick_stops_summary", L.TickStopsSummary, 24),
                                ("wa_axes_dwells_summary", L.AxesDwellsSummary, 40)):
        assert struct_fields(code, cname) == [f for f, _ in struct._fields_], cname
        assert C.sizeof(struct) == size, cname
    assert L.AxesDwellsSummary.max_need.offset == 32 and dict(L.AxesDwellsSummary._fields_)["max_need"] is C.c_double
    # the argument counts of the header's prototypes
    for name in CALLS:
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(L.SYMBOLS[name][1]), name
    assert len(L.SYMBOLS["wa_traj_retime_stops"][1]) == len(L.SYMBOLS["wa_traj_retime"][1]) + 2
    assert len(L.SYMBOLS["wa_traj_tick_axes_stops"][1]) == len(L.SYMBOLS["wa_traj_tick_axes"][1]) + 3


def test_null_arguments_are_answered_not_followed(lib):
    assert lib.wa_traj_retime_stops(None, None, None, None, None, 0.01, None, None, None, None, None, None) == ARG
    assert lib.wa_traj_tick_axes_stops(None, None, None, None, -1, 1.0, 1.0, 0.01, None, None, None, None, None, None, None, None) == ARG
    assert lib.wa_traj_axes_dwells(None, None, 1.0, None, None, None) == ARG


def test_python_wrappers_exist():
    for name in ("retime_stops", "axis_dwells", "tick_axes_stops"):
        assert callable(getattr(api.Trajectory, name)), name


def test_plan_batch_refuses_weld_passes_without_seams():
    exe = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py")]
    r = subprocess.run(exe + ["--weld-passes", "0.5", "0.2", "0.1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--seams" in r.stderr, r.stderr[-300:]
    r = subprocess.run(exe + ["--seams", "--weld-passes", "0.5", "0.2", "0.1", "--torch", "8", "--retime", "--tick-poses", "1.0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr[-300:]
