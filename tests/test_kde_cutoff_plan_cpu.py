"""CPU: the pure parts of pdfz::EvalKernel's cutoff radius (sxmc_amd/csrc/kde_cutoff.h) from a stand-alone program,
plain and under ASan + UBSan (tests/cpp/test_kde_cutoff_plan.cpp: the order is a stable permutation, boxes of
constructed tiles, the visit test monotone in R and never rejecting a tile that holds a pair below qcut, the edge
cases); the new C ABI entry points declared, exported, in the ctypes table and on the Python class; and invalid R
refused before any device work."""
import ctypes as C
import math
import os
import subprocess

import pytest

from sxmc_amd import capi, pdfz
from tests.test_abi import declared_symbols, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"sxmc_kde_set_cutoff", "sxmc_kde_cutoff", "sxmc_kde_cutoff_stats", "sxmc_kde_cutoff_boxes",
                    "sxmc_kde_pair_split"}


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "test_kde_cutoff_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_kde_cutoff_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, src], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_kde_cutoff_plan: ok" in r.stdout, r.stdout + r.stderr


def test_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    assert NEW_ENTRY_POINTS <= set(declared_symbols())
    assert NEW_ENTRY_POINTS <= exported(capi.LIB_PATH)
    assert NEW_ENTRY_POINTS <= set(capi.SIGNATURES)
    for name in ("SetCutoff", "Cutoff", "CutoffStats", "PairSplit"):
        assert callable(getattr(pdfz.EvalKernel, name))


def test_invalid_radii_are_refused_without_a_device():
    lib = capi.load()
    for R in (math.nan, -1.0, 0.5, 0.999999, -math.inf, 1e-300):
        assert lib.sxmc_kde_set_cutoff(None, R) == capi.ERR_INVALID
        assert capi.last_error() == "Bandwidth cutoff must be 0 or a number >= 1 (infinity allowed)."
    for R in (0.0, 1.0, 3.0, math.inf):                       # a valid R gets as far as the evaluator
        assert lib.sxmc_kde_set_cutoff(None, R) == capi.ERR_INVALID
        assert capi.last_error() == "null evaluator"
    v = C.c_double(7.0)
    assert lib.sxmc_kde_cutoff(None, C.byref(v)) == capi.ERR_INVALID
    a, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert lib.sxmc_kde_cutoff_stats(None, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    n, t = C.c_int(0), C.c_uint(0)
    assert lib.sxmc_kde_pair_split(None, C.byref(n), C.byref(t)) == capi.ERR_INVALID
