"""CPU, no device: who owns the library's device memory.

tests/cpp/test_device_buffer.cpp drives sxmc_amd/csrc/device_buffer.h -- the one buffer type every handle of the host side
holds its allocations in -- over a host policy that logs every call, keeps the set of live blocks and fails the k-th
allocation on demand: moves, grow-only growth (free first, then allocate; nothing when the request fits), retiring, and a
fault-injection sweep over a creation and a growth of four buffers.  A plain build and one under AddressSanitizer +
UndefinedBehaviorSanitizer (a failed allocation cannot be provoked on a GPU; here it is swept).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "sxmc_amd", "csrc")


@pytest.mark.parametrize("exe", ["test_device_buffer", "test_device_buffer_asan"])
def test_device_buffer_device_free(exe):
    subprocess.check_call(["make", "-s", "-C", CPP, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CPP, exe)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "9 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_buffer_header_needs_no_hip(tmp_path):
    """device_buffer.h is what every handle of the host side owns its memory through: it must stay free of HIP and of
    library state, or the device-free test above stops covering what runs in production."""
    text = open(os.path.join(CSRC, "device_buffer.h")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())      # (comments may name HIP)
    assert "hip" not in code.lower() and "#include <hip" not in text
    # ... and compiles by itself, with no HIP include path (-nostdinc++ would go too far: it uses <cstddef>, <type_traits>)
    src = tmp_path / "alone.cpp"
    src.write_text('#include "device_buffer.h"\nint main() { return 0; }\n')
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", CSRC, str(src)])
    # the library's handles are built on it, through the policies sxmc_host.h gives
    host = open(os.path.join(CSRC, "sxmc_host.h")).read()
    assert '#include "device_buffer.h"' in host and "sxbuf::Buffer<T, DeviceMem>" in host
