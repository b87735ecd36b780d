"""The torch-axis stage at the product boundary, without a device: the header declares the two calls, the library exports them, the
bindings match the header's structs, the calls answer NULL arguments with WA_ERR_ARG, the Python wrappers exist and
examples/plan_batch.py knows --torch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import torch_ref as T
from welding_robot_amd import _lib as L
from welding_robot_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


def _struct(code, name):
    return code.split(name + ";")[0].rsplit("typedef struct", 1)[1]


def test_header_declares_and_library_exports_the_calls(lib):
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("wa_traj_tool_axes", "wa_traj_tool_check"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define\s+WA_TORCH_MAX_DIRS\s+256\b", code) and re.search(r"#define\s+WA_TORCH_MAX_BEADS\s+64\b", code)
    assert (L.TORCH_MAX_DIRS, L.TORCH_MAX_BEADS, L.TORCH_INF, api.TORCH_INF) == (256, 64, 1 << 62, 1 << 62)
    names = re.findall(r"\b(\w+)\s*(?:\[\w+\])?\s*[,;]", _struct(code, "wa_tool_beads"))
    assert names == [f for f, _ in L.ToolBeads._fields_] == ["n_beads", "dist16", "r2"]
    assert C.sizeof(L.ToolBeads) == 4 + 2 * 64 * 4 and L.ToolBeads.dist16.offset == 4 and L.ToolBeads.r2.offset == 4 + 256
    names = re.findall(r"\b(\w+)\s*[,;]", _struct(code, "wa_tool_weights"))
    assert names == [f for f, _ in L.ToolWeights._fields_] and C.sizeof(L.ToolWeights) == 20
    names = re.findall(r"\b(\w+)\s*[,;]", _struct(code, "wa_tool_summary"))
    assert names == [f for f, _ in L.ToolSummary._fields_] == list(T.SUMMARY_FIELDS) and C.sizeof(L.ToolSummary) == 80
    # the argument order of the two declarations
    args = re.search(r"int\s+wa_traj_tool_axes\s*\((.*?)\)\s*;", code, re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", args) == ["g", "t", "dirs", "K", "tool", "weights", "want", "off", "n_legs", "pin_first", "pin_last",
                                                     "dir_out", "feas_out", "leg_cost", "sum"]
    assert len(L.SYMBOLS["wa_traj_tool_axes"][1]) == 15
    args = re.search(r"int\s+wa_traj_tool_check\s*\((.*?)\)\s*;", code, re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", args) == ["g", "t", "axes", "tool", "near_add", "blocked_out", "near_out", "sum"]
    assert len(L.SYMBOLS["wa_traj_tool_check"][1]) == 8


def test_null_arguments_are_answered_not_followed(lib):
    assert lib.wa_traj_tool_axes(None, None, None, 0, None, None, None, None, 0, None, None, None, None, None, None) == ARG
    assert lib.wa_traj_tool_check(None, None, None, None, 0, None, None, None) == ARG


def test_python_wrappers_exist():
    assert callable(api.Trajectory.torch_axes) and callable(api.Trajectory.torch_check) and callable(api.torch_cone) and callable(api.torch_tool)
    d = api.torch_cone(64, 1.2, (0.3, -0.2, 1.0))
    assert d.shape == (64, 3) and d.dtype == np.float32 and np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    a = np.float64([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    assert np.allclose(d[0], a, atol=1e-6) and (d @ a >= np.cos(1.2) - 1e-6).all()
    assert np.array_equal(d, T.fib_dirs(64, 1.2, (0.3, -0.2, 1.0)))
    assert api.torch_cone(1, 0.5).tolist() == [[0.0, 0.0, 1.0]]
    t = api.torch_tool([0, 16, 32], [1, 2, 3])
    assert t.n_beads == 3 and list(t.dist16[:3]) == [0, 16, 32] and list(t.r2[:4]) == [1, 2, 3, 0]
    with pytest.raises(ValueError):
        api.torch_tool([], [])
    with pytest.raises(ValueError):
        api.torch_tool([0] * 65, [0] * 65)


def test_plan_batch_refuses_what_torch_cannot_do():
    exe = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py")]
    for extra, word in (([], "--fit"), (["--fit", "--shortcut", "--safe-paths", "3", "--torch", "0"], "1 .. 256"),
                        (["--fit", "--shortcut", "--safe-paths", "3", "--torch", "257"], "1 .. 256")):
        r = subprocess.run(exe + (["--torch"] if "--torch" not in extra else []) + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr[-300:])
