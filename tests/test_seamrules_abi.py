"""Seam tours under job rules at the product boundary, without a device: the header declares the three calls, the library exports them,
the summary struct matches, NULL arguments are answered with WA_ERR_ARG, wa_gtsp_seam_rules_check (host only) agrees with the restatement
on hand-made tours, and examples/plan_batch.py knows --seam-before / --seam-fixed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import seamrules_ref as S
from welding_robot_amd import _lib as L
from welding_robot_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1
NAMES = ("wa_gtsp_seam_tour_rules", "wa_gtsp_seam_tour_rules_exact", "wa_gtsp_seam_rules_check")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        build.build()
    return L.load()


def test_header_declares_and_library_exports_the_calls(lib):
    hdr = open(os.path.join(ROOT, "include", "weldacs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    names = re.findall(r"\b(\w+)\s*[,;]", code.split("wa_seam_rules_summary;")[0].rsplit("typedef struct", 1)[1])
    assert names == [f for f, _ in L.SeamRulesSummary._fields_]
    # wa_seam_summary's fields at wa_seam_summary's offsets, then two int32
    assert names[:len(L.SeamSummary._fields_)] == [f for f, _ in L.SeamSummary._fields_] and names[-2:] == ["n_prec", "n_fixed"]
    for f, _ in L.SeamSummary._fields_:
        assert getattr(L.SeamRulesSummary, f).offset == getattr(L.SeamSummary, f).offset
    assert C.sizeof(L.SeamRulesSummary) == 64 and L.SeamRulesSummary.n_prec.offset == 56 and L.SeamRulesSummary.n_fixed.offset == 60
    # the argument lists of the header, type by type
    for name in NAMES:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)
        args = [a.strip() for a in decl.split(",")]
        assert len(args) == len(L.SYMBOLS[name][1]), name
        for a, t in zip(args, L.SYMBOLS[name][1]):
            assert ("*" in a) == (t is C.c_void_p or hasattr(t, "contents")), (name, a)


def test_null_arguments_are_answered_not_followed(lib):
    assert lib.wa_gtsp_seam_tour_rules(None, None, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == ARG
    assert lib.wa_gtsp_seam_tour_rules_exact(None, None, 0, 0, None, None, 0, None, None, None, None) == ARG
    assert lib.wa_gtsp_seam_rules_check(None, 0, 0, None, None, 0, None, None, None, None, None) == ARG


def test_python_wrappers_exist():
    assert callable(api.seam_tour_rules) and callable(api.seam_tour_rules_exact) and callable(api.seam_rules_check)


def test_check_counts_what_a_tour_breaks(lib):
    # 5 seams: 1 before 2 (given twice), 3 before 1, seam 2 only from its odd end, seam 4 only from its even end
    before, after, fixed = [1, 3, 1], [2, 1, 2], [0, 0, 2, 0, 1]
    tours = [([0, 3, 1, 2, 4], [0, 1, 0, 1, 0]), ([0, 1, 2, 3, 4], [0, 0, 0, 0, 0]), ([0, 2, 1, 3, 4], [1, 1, 1, 1, 1]),
             ([4, 2, 0, 3, 1], [0, 0, 0, 0, 0]), ([3, 1, 2, 4, 0], [1, 0, 1, 0, 1])]
    seen = set()
    for closed in (True, False):
        for order, dirs in tours:
            want = S.check(5, closed, before, after, fixed, order, dirs)
            assert api.seam_rules_check(order, dirs, before, after, fixed, closed=closed) == want
            seen.add(want)
    assert (0, 0) in seen and len(seen) >= 4
    assert api.seam_rules_check([1, 2, 0, 3, 4], [0, 1, 0, 0, 0], before, after, fixed, closed=True) == (0, 0)   # read from seam 0
    assert api.seam_rules_check([1, 2, 0, 3, 4], [0, 1, 0, 0, 0], before, after, fixed, closed=False) == (1, 0)
    assert api.seam_rules_check([0, 2, 1, 3, 4], [0, 0, 0, 0, 1], before, after, fixed, closed=True) == (3, 2)
    assert api.seam_rules_check([0, 1], [0, 1], closed=True) == (0, 0)   # no rules, nothing to break

    def rc(m=5, closed=1, before=before, after=after, fixed=fixed, order=(0, 3, 1, 2, 4), dirs=(0, 1, 0, 1, 0), n_prec=None, null=()):
        b, a = np.array(before, np.int32), np.array(after, np.int32)
        f, o, d = np.array(fixed, np.uint8), np.array(order, np.int32), np.array(dirs, np.uint8)
        out = np.full(2, -7, np.int64)
        ptr = lambda name, x: None if name in null else x.ctypes.data
        r = lib.wa_gtsp_seam_rules_check(None, m, closed, ptr("before", b), ptr("after", a), len(b) if n_prec is None else n_prec, ptr("fixed", f),
                                         ptr("order", o), ptr("dir", d), None if "bad_p" in null else out[0:].ctypes.data,
                                         None if "bad_d" in null else out[1:].ctypes.data)
        return r, bool((out == -7).all())

    assert rc() == (0, False)
    assert rc(null=("fixed",))[0] == 0
    bad = [rc(null=(n,)) for n in ("before", "after", "order", "dir", "bad_p", "bad_d")]
    bad += [rc(m=0), rc(m=1025), rc(n_prec=-1), rc(n_prec=65537), rc(before=[1, 3, 5]), rc(after=[2, 1, -1]), rc(before=[1, 3, 2]),
            rc(before=[1, 2, 3], after=[2, 3, 1]), rc(after=[2, 1, 0]), rc(fixed=[0, 0, 3, 0, 0]), rc(order=(0, 3, 1, 2, 2)),
            rc(order=(0, 3, 1, 2, 5)), rc(dirs=(0, 1, 0, 1, 2))]
    for r in bad:
        assert r == (ARG, True), bad.index(r)
    assert rc(closed=0, after=[2, 1, 0])[0] == 0   # an open tour may put a seam before seam 0


def test_plan_batch_knows_the_rule_flags():
    exe = [sys.executable, os.path.join(ROOT, "examples", "plan_batch.py")]
    for extra, word in ((["--seam-before", "1:2"], "--seams"), (["--seams", "--seam-before", "1:0"], "seam 0"),
                        (["--seams", "--seam-before", "1-2"], "N:N"), (["--seams", "--seam-fixed", "1:2"], "direction"),
                        (["--seams", "--points", "8", "--seam-fixed", "4:0"], "0 .. 3"),
                        (["--seams", "--points", "7", "--seam-before", "1:2"], "even"),
                        (["--seams", "--retime", "--seam-fixed", "1:0"], "--retime")):
        r = subprocess.run(exe + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr[-300:])
    r = subprocess.run(exe + ["--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--seam-before" in r.stdout and "--seam-fixed" in r.stdout
