"""CPU, no device: how the multi-GPU runner shares experiments among ranks and brings their intervals back
(sxmc_amd/include/sxmc/ensemble_plan.h -- rank k mod G, blocks of ceil(N / G) slots padded with NaN, the reorder into
experiment order, the medians) and the meeting points of the runners' host threads (lane_sync.h: LaneBarrier,
Rendezvous), swept by tests/cpp/test_ensemble_plan.cpp in a plain build and under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
INCLUDE = os.path.join(ROOT, "sxmc_amd", "include", "sxmc")


@pytest.mark.parametrize("exe", ["test_ensemble_plan", "test_ensemble_plan_asan"])
def test_shards_blocks_and_meeting_points_device_free(exe):
    subprocess.check_call(["make", "-s", "-C", CPP, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CPP, exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "5 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _code(name):
    text = open(os.path.join(INCLUDE, name)).read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)      # (comments may name entry points)


def test_the_pure_headers_need_no_library():
    """ensemble_plan.h, lane_sync.h and chain.h stand on the standard library alone and intervals.h on chain.h, or the
    device-free sweep above (and intervals_dump's sanitizer build) stops covering what runs in production."""
    for name in ("ensemble_plan.h", "lane_sync.h", "chain.h"):
        code = _code(name)
        assert not re.search(r'#include\s*"', code), name + " includes a project header"
        assert "sxmc_" not in code and "hip" not in code.lower() and "pdfz" not in code, name
    code = _code("intervals.h")
    assert re.findall(r'#include\s*"([^"]+)"', code) == ["chain.h"]
    assert "sxmc_" not in code and "hip" not in code.lower() and "pdfz" not in code
    # ... and the multi-GPU runner calls the plan, keeping no second copy of its arithmetic
    used = _code("multi_gpu.h")
    assert '#include "ensemble_plan.h"' in used
    for fn in ("experiments_of(", "pack(", "unpack(", "median_upper(", "empty_blocks("):
        assert "plan." + fn in used, fn + " is not what ensemble_multi_gpu calls"
    assert "% G" not in used and "/ G" not in used and "quiet_NaN" not in used
