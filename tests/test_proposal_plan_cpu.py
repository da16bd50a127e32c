"""CPU, no device: the correlated proposal in the C++ walk's plan (sxmc_amd/include/sxmc/walk_plan.h) -- a walk with
covariance_proposal never takes the look-ahead pass or a lockstep set's step, every other fact's outcome is unchanged --
swept by tests/cpp/test_proposal_plan.cpp in a plain build and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("exe", ["test_proposal_plan", "test_proposal_plan_asan"])
def test_proposal_plan_device_free(exe):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "proposal.mk", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CPP, exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "2 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
