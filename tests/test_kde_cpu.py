"""CPU: pdfz::EvalKernel's C ABI is declared and exported, its constructor validation (which needs no GPU) raises the
contract's messages, and the C++ walk over a kernel-density signal compiles with the C++ tests' flags and, without a
device, says so."""
import os
import re
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, pdfz
from tests.test_abi import declared_symbols, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KDE_ENTRY_POINTS = {"sxmc_kde_" + n for n in (
    "create", "destroy", "add_systematic", "set_eval_points", "set_pdf_value_buffer", "set_normalization_buffer",
    "set_parameter_buffer", "eval_async", "eval_finished", "get_stream", "bandwidths", "nsamples", "npoints")}


def test_header_declares_and_library_exports_the_kde_entry_points():
    assert KDE_ENTRY_POINTS <= set(declared_symbols())
    assert KDE_ENTRY_POINTS <= exported(capi.LIB_PATH)
    assert KDE_ENTRY_POINTS <= set(capi.SIGNATURES)
    lib = capi.load()
    for n in KDE_ENTRY_POINTS:
        assert getattr(lib, n) is not None


def kde_error(**kw):
    a = dict(samples=np.linspace(0.0, 1.0, 8, dtype=np.float32), nfields=1, nobservables=1, lower=[0.0],
             upper=[1.0], bandwidth_scale=[1.0])
    a.update(kw)
    with pytest.raises(pdfz.Error) as e:
        pdfz.EvalKernel(**a)
    return e.value.msg


def test_constructor_messages_match_eval():
    # Eval::Eval's checks, pdfz.cpp:64-82, in its order
    assert kde_error(samples=np.zeros(7, np.float32), nfields=2) == \
        "Length of samples array is not divisible by number of fields."
    assert kde_error(nobservables=0) == "Number of observables in PDF is zero."
    assert kde_error(nobservables=2) == "Number of observables cannot be greater than number of fields."
    assert kde_error(upper=[1.0, 2.0]) == "Number of upper bounds must be same as number of observables."
    assert kde_error(lower=[0.0, 0.0]) == "Number of lower bounds must be same as number of observables."
    assert "MAX_NFIELDS" in kde_error(samples=np.zeros(22, np.float32), nfields=11)


def test_constructor_bandwidth_scale_and_dimension_checks():
    assert kde_error(bandwidth_scale=[1.0, 1.0]) == "Number of bandwidth scales must be same as number of observables."
    assert kde_error(bandwidth_scale=[]) == "Number of bandwidth scales must be same as number of observables."
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "positive and finite" in kde_error(bandwidth_scale=[bad])
    five = dict(samples=np.random.default_rng(1).random(50, dtype=np.float32), nfields=5, nobservables=5,
                lower=[0.0] * 5, upper=[1.0] * 5, bandwidth_scale=[1.0] * 5)
    assert "at most 4 observables" in kde_error(**five)
    assert "Upper bound must be greater" in kde_error(upper=[0.0])


def test_constructor_bandwidth_needs_spread():
    assert "at least 2 samples" in kde_error(samples=np.array([0.5, 3.0, -1.0], np.float32))
    assert "no spread" in kde_error(samples=np.full(10, 0.25, np.float32))
    # NaN and out-of-domain rows do not count
    assert "at least 2 samples" in kde_error(samples=np.array([0.5, np.nan, 1.0, 2.0], np.float32))


def cpp_flags():
    """The compile and link flags of tests/cpp/Makefile (CXXFLAGS, LDFLAGS), read from it."""
    text = open(os.path.join(ROOT, "tests", "cpp", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS = (.*)$", text, flags=re.M).group(1)
    ld = re.search(r"^LDFLAGS = (.*)$", text, flags=re.M).group(1)
    cxx = cxx.replace("$(ROOT)", os.path.join(ROOT))
    csrc = os.path.join(ROOT, "sxmc_amd", "csrc")
    ld = ld.replace("$(ROOT)", ROOT).replace("'$$ORIGIN/../../sxmc_amd/csrc'", csrc)
    return cxx.split(), ld.split()


def build_kde_walk(outdir):
    cxx, ld = cpp_flags()
    exe = os.path.join(str(outdir), "test_kde_walk")
    src = os.path.join(ROOT, "tests", "cpp", "test_kde_walk.cpp")
    subprocess.run(["g++"] + cxx + ["-o", exe, src] + ld, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_kde_walk_compiles_and_needs_a_device(tmp_path):
    exe = build_kde_walk(tmp_path)
    if capi.device_count() > 0:
        return   # (with a device the walk runs: tests/test_gpu_kde.py)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no GPU device" in r.stdout
