"""CPU: the pure parts of pdfz::EvalKernel's evaluation plan (sxmc_amd/csrc/kde_plan.h) from a stand-alone program,
plain and under ASan + UBSan (tests/cpp/test_kde_plan.cpp: the pair sum's split against pinned values and a brute-force
search, the in-domain rows of a row-major and a column-major view of one table with rows on the edges, NaN and the
infinities, the projection's split, and the truncation mass against the expression typed out)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "test_kde_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_kde_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, src], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_kde_plan: ok" in r.stdout, r.stdout + r.stderr
