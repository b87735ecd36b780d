"""The seam-tour stage at the product boundary, without a device: the header declares the two calls, the library exports them, the
bindings match the header's structs, the calls answer NULL arguments with WA_ERR_ARG, and examples/plan_batch.py knows --seams."""
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


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


def test_header_declares_and_library_exports_the_calls(lib):
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("wa_gtsp_seam_tour", "wa_gtsp_seam_tour_exact"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    for field in ("closed", "or_len", "n_starts", "max_passes", "seed"):
        assert re.search(r"\b%s\b" % field, code.split("wa_seam_params;")[0].rsplit("typedef struct", 1)[1])
    assert [f for f, _ in L.SeamParams._fields_] == ["closed", "or_len", "n_starts", "max_passes", "seed"]
    assert C.sizeof(L.SeamParams) == 24 and L.SeamParams.seed.offset == 16
    # five int32, padding to 8, four int64
    assert C.sizeof(L.SeamSummary) == 56 and L.SeamSummary.cost_q.offset == 24 and L.SeamSummary.passes_total.offset == 48
    names = re.findall(r"\b(\w+)\s*[,;]", code.split("wa_seam_summary;")[0].rsplit("typedef struct", 1)[1])
    assert names == [f for f, _ in L.SeamSummary._fields_]


def test_null_arguments_are_answered_not_followed(lib):
    assert lib.wa_gtsp_seam_tour(None, None, 0, None, None, None, None, None, None, None, None) == ARG
    assert lib.wa_gtsp_seam_tour_exact(None, None, 0, 0, None, None, None) == ARG


def test_python_wrappers_exist():
    assert callable(api.seam_tour) and callable(api.seam_tour_exact) and api.SEAM_Q == 1 << 20


def test_plan_batch_refuses_what_seams_cannot_do():
    exe = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py")]
    for extra, word in ((["--points", "7"], "even"), (["--retime"], "--retime"), (["--shortcut", "--fit"], "--fit")):
        r = subprocess.run(exe + ["--seams"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr[-300:])
