"""CPU, no device: the schedule of the C++ walk (sxmc_amd/include/sxmc/walk_plan.h -- which steps end a run, where the
widths are re-tuned, how a run splits into graph replays and a remainder, the rounds of the look-ahead walk, the form
of the steps) swept by tests/cpp/test_walk_plan.cpp, in a plain build and under AddressSanitizer +
UndefinedBehaviorSanitizer; and the same flush rule in Python (sxmc_amd.mcmc.flush_due) against the C++ one."""
import os
import re
import subprocess

import pytest

from sxmc_amd import mcmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
HEADER = os.path.join(ROOT, "sxmc_amd", "include", "sxmc", "walk_plan.h")


def _make(target):
    subprocess.check_call(["make", "-s", "-C", CPP, target])


@pytest.mark.parametrize("exe", ["test_walk_plan", "test_walk_plan_asan"])
def test_walk_schedule_device_free(exe):
    _make(exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CPP, exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "6 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_python_and_cpp_flush_the_same_steps():
    """The two languages differ only in when they consider a plan to have two forms; that input is passed in."""
    _make("test_walk_plan")
    for nsteps, burnin in ((0, 0), (1, 0), (40, 0), (40, 8), (41, 20), (333, 66), (100, 50)):
        for sync, adapt in ((7, 5), (16, 1), (100, 5), (100, 30), (2, 1), (1000, 7)):
            assert adapt < sync
            for two_forms in (False, True):
                r = subprocess.run([os.path.join(CPP, "test_walk_plan"), "--dump", str(nsteps), str(burnin), str(sync),
                                    str(adapt), str(int(two_forms))], capture_output=True, text=True, timeout=60)
                assert r.returncode == 0, r.stderr[-2000:]
                want = [i for i in range(nsteps) if mcmc.flush_due(i, nsteps, burnin, sync, adapt, two_forms)]
                assert [int(t) for t in r.stdout.split()] == want, (nsteps, burnin, sync, adapt, two_forms)


def test_flush_schedule_is_flush_due_at_every_step():
    """MCMC.flush_schedule asks flush_due only where one of its terms can hold; the list is the one a walk over every
    step gives."""
    class Chain:
        def __init__(self, nsteps, burnin, sync, two_forms):
            self._nsteps, self._burnin, self.sync_interval, self._two = nsteps, burnin, sync, two_forms

        def _two_forms(self):
            return self._two

    for nsteps, burnin in ((0, 0), (1, 0), (40, 0), (40, 8), (41, 20), (333, 66), (2500, 500), (3001, 1500)):
        for sync in (1, 7, 100, 1500, 10000):
            for two_forms in (False, True):
                want = [i for i in range(nsteps)
                        if mcmc.flush_due(i, nsteps, burnin, sync, mcmc.ADAPT_INTERVAL, two_forms)]
                assert mcmc.MCMC.flush_schedule(Chain(nsteps, burnin, sync, two_forms)) == want


def test_walk_plan_header_needs_no_library():
    """walk_plan.h is what mcmc.h schedules a walk from: it must stay free of the library and of every other project
    header, or the device-free sweep above stops covering what runs in production."""
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)      # (comments may name entry points)
    assert not re.search(r'#include\s*"', code), "walk_plan.h includes a project header"
    assert "sxmc_" not in code and "hip" not in code.lower()
    used = open(os.path.join(ROOT, "sxmc_amd", "include", "sxmc", "mcmc.h")).read()
    assert '#include "walk_plan.h"' in used
    for fn in ("run_end", "retune_due", "split_run", "lookahead_round", "choose_form"):
        assert fn + "(" in used, fn + " is not what the walk calls"
    # ... and the walk keeps no second copy of the flush rule
    assert "% sync_interval" not in used and "% plan.sync_interval" not in used
