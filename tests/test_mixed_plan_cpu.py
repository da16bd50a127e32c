"""CPU, no device: what a MIXED walk (histogram + kernel-density signals in one batched, recordable step) decides and
refuses before any launch -- tests/cpp/test_mixed_plan.cpp (the form of the steps over every flag combination, the
column table of sxmc_group_set_columns, the null-handle answers of the new entry points), in a plain build and under
AddressSanitizer + UndefinedBehaviorSanitizer -- and that the new entry points are declared, exported and in the ctypes
table, with their Python spellings."""
import os
import re
import subprocess

import pytest

from sxmc_amd import capi, nll, pdfz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

NEW_ENTRIES = ("sxmc_kde_eval_on_stream_async", "sxmc_kde_parameters_read", "sxmc_kde_evaluation_count",
               "sxmc_group_set_columns", "sxmc_group_eval_columns_nll_async", "sxmc_group_finish_columns_step_async")


@pytest.mark.parametrize("exe", ["test_mixed_plan", "test_mixed_plan_asan"])
def test_mixed_plan_without_a_device(exe):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "mixed.mk", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CPP, exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "5 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_new_entries_are_declared_exported_and_in_the_ctypes_table():
    header = open(os.path.join(ROOT, "include", "sxmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = capi.load()
    out = os.popen("nm -D --defined-only %s" % capi.LIB_PATH).read()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in capi.SIGNATURES, name + " is not in the ctypes table"
        assert getattr(lib, name).argtypes == capi.SIGNATURES[name]
    # the argument lists of the two step entries are their neighbours' (a stream, then the reference's lists)
    assert len(capi.SIGNATURES["sxmc_group_finish_columns_step_async"]) == len(
        capi.SIGNATURES["sxmc_group_finish_step_async"])
    assert len(capi.SIGNATURES["sxmc_group_eval_columns_nll_async"]) == 12


def test_python_spellings_exist_and_refuse_null_handles():
    for cls, names in ((pdfz.EvalKernel, ("EvalOnStream", "ParametersRead", "EvaluationCount")),
                       (nll.EvalGroup, ("SetColumns", "EvalColumnsNllAsync", "FinishColumnsStepAsync"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    lib = capi.load()
    assert lib.sxmc_group_set_columns(None, 1, None) == capi.ERR_INVALID
    assert b"null group" in lib.sxmc_last_error()
    assert lib.sxmc_kde_eval_on_stream_async(None, 1, None) == capi.ERR_INVALID
    assert lib.sxmc_kde_parameters_read(None, None, 0, None) == capi.ERR_INVALID
    assert lib.sxmc_kde_evaluation_count(None, None) == capi.ERR_INVALID


def test_the_walk_takes_its_form_from_the_planner():
    """mcmc.h passes the new flag to choose_form and launches the mixed step through the new entries only."""
    used = open(os.path.join(ROOT, "sxmc_amd", "include", "sxmc", "mcmc.h")).read()
    assert "!m.kernels.empty()});" in used
    for name in ("sxmc_kde_eval_on_stream_async", "sxmc_group_eval_columns_nll_async",
                 "sxmc_group_finish_columns_step_async", "sxmc_group_set_columns", "sxmc_kde_parameters_read"):
        assert name + "(" in used, name
