"""CPU: the pure parts of the end of a Metropolis step (sxmc_amd/csrc/step_end_plan.h) from a stand-alone program, plain
and under ASan + UBSan (tests/cpp/test_step_end_plan.cpp: the blocks of the event sum, the chunks of the clearing and the
kernels' LDS size against pinned values and the expressions typed out, the words of the ticket block distinct and inside
it); and that the header stays free of HIP, or the program stops covering what the library runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "test_step_end_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_step_end_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, src], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_step_end_plan: ok" in r.stdout, r.stdout + r.stderr


def test_plan_header_needs_no_hip():
    text = open(os.path.join(ROOT, "sxmc_amd", "csrc", "step_end_plan.h")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())      # (comments may name HIP)
    assert "hip" not in code.lower()
