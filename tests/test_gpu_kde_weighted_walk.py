"""GPU: a small mixed fit of sxmc::MCMC -- one histogram signal, one kernel-density signal that floats both systematics,
300 events, 300 steps through both re-tunings -- whose kernel signal carries every multiplicity 8 (n_mc = 8 n, set by
build_pdfz) gives the chain BYTES of the same fit with the kernel signal unweighted: in the reference form, with the MIXED
defaults and in graphs of 16 steps (tests/cpp/kde_weights_walk.cpp).  build_pdfz refuses the row-count mismatch and the
combination with cross-validation by name."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_walks_and_refusals():
    exe = os.path.join(ROOT, "tests", "cpp", "kde_weights_walk")
    assert os.access(exe, os.X_OK), exe + " is missing: __graft_entry__.build() makes it (tests/cpp/kdeweights.mk)"
    done = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
    said = done.stdout
    for form in ("reference_form", "mixed", "graphs_of_16", "row_count_refused", "cv_refused"):
        assert ("ok " + form + "\t") in said, said
    assert "forms mixed mixed" in [l for l in said.splitlines() if l.startswith("ok mixed")][0], said
