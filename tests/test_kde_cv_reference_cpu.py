"""CPU: bandwidth cross-validation of pdfz::EvalKernel where no device is needed -- self-checks of the numpy reference
(tests/kde_cv_reference.py) every GPU test compares with, the gap condition of the selection cases those tests repeat,
the host arithmetic (sxmc_amd/csrc/kde_cv.h) from a stand-alone program, plain and under ASan + UBSan, that program's
grid, split and subset against the reference's restatement, and the new C ABI entry points declared, exported, in the
ctypes table and refusing bad arguments before any device work."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, pdfz
from tests import kde_cv_reference as cv
from tests.test_abi import declared_symbols, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"sxmc_kde_cv_scores", "sxmc_kde_cv_select", "sxmc_kde_bandwidth_scale"}
HOST_FLAGS = {"plain": ["-O2"], "asan-ubsan": ["-O1", "-g", "-fsanitize=address,undefined",
                                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]}


# ------------------------------------------------------------------ the reference checks itself
@pytest.mark.parametrize("m,D", [(2, 1), (3, 2), (5, 3), (8, 4), (8, 1)])
def test_reference_against_a_plain_double_loop(m, D):
    x, lower, upper = cv.table_with_inside(70 + m + D, m, D)
    rows, n, sigma = cv.scored_rows(x.ravel(), x.shape[1], D, lower, upper)
    assert n == m and len(rows) == m
    for s in (0.3, 1.0, 2.5):
        h = cv.candidates([[s] * D], sigma, m)[0]
        got, bound = cv.scores(rows, lower, upper, [h])
        want = cv.scores_double_loop(rows.tolist(), lower, upper, h.tolist())
        assert math.isfinite(want) and abs(got[0] - want) <= 2 * bound[0], (got[0], want, bound[0])
        assert bound[0] < 1e-12


def test_closed_form_for_two_rows_in_one_dimension():
    lower, upper = np.array([-1.0]), np.array([3.0])
    a, b, h = 0.25, 1.5, 0.7
    rows = np.array([[a], [b]])

    def Phi(z):
        return 0.5 * math.erfc(-z / math.sqrt(2.0))

    def lnf(other):      # the one term of a row's sum: the other row's truncated kernel at this row
        M = Phi((upper[0] - other) / h) - Phi((lower[0] - other) / h)
        return -0.5 * ((a - b) / h) ** 2 - math.log(h * M * math.sqrt(2.0 * math.pi))

    want = 0.5 * (lnf(b) + lnf(a))
    got, bound = cv.scores(rows, lower, upper, [[h]])
    assert abs(got[0] - want) <= 2 * bound[0] + 4 * cv.EPS * abs(want)


def test_a_candidate_that_leaves_a_row_without_neighbours_scores_minus_infinity():
    x, lower, upper = cv.table_with_inside(5, 40, 2)
    rows, _, sigma = cv.scored_rows(x.ravel(), 2, 2, lower, upper)
    h = cv.candidates([[1.0, 1.0], [1e-4, 1e-4], [0.5, 0.5]], sigma, len(rows))
    got, bound = cv.scores(rows, lower, upper, h)
    assert math.isfinite(got[0]) and got[1] == -math.inf and math.isfinite(got[2])
    g = [1.0, 1e-4, 0.5]
    assert cv.choose(g, got) in (0, 2)
    assert cv.choose(g, [-math.inf] * 3) == -1 and cv.choose(g, [math.nan, -math.inf, math.inf]) == -1
    with pytest.raises(ValueError, match="no finite score"):
        cv.search(cv.Options(lo=1e-5, hi=1e-4, steps=3), 2,
                  lambda mult: cv.scores(rows, lower, upper, cv.candidates(mult, sigma, len(rows)))[0])


def test_reference_error_is_far_below_the_bound():
    """The f64 reference against the same sums, exp and ln in np.longdouble (the masses stay f64)."""
    for D, m in ((1, 300), (2, 257), (4, 120)):
        x, lower, upper = cv.table_with_inside(90 + D, m, D)
        rows, _, sigma = cv.scored_rows(x.ravel(), D, D, lower, upper)
        h = cv.candidates([[s] * D for s in (0.25, 1.0, 4.0)], sigma, m)
        f64, bound = cv.scores(rows, lower, upper, h)
        ext, _ = cv.scores(rows, lower, upper, h, dtype=np.longdouble)
        err = np.abs(f64 - ext)
        print("D=%d m=%d: reference error %s, bound %s" % (D, m, err, bound))
        assert np.all(err <= 0.1 * bound) and np.all(bound < 1e-12)


def test_ties_and_the_choice():
    assert cv.choose([0.25, 0.5, 2.0], [-1.0, -1.0, -1.0]) == 1
    assert cv.choose([2.0, 0.5], [-1.0, -1.0]) == 1 and cv.choose([0.5, 1.0, 2.0], [-3.0, -2.0, -2.5]) == 1


def run_search(x, nobs, lower, upper, o):
    return cv.select(x.ravel(), x.shape[1], nobs, lower, upper, o)


@pytest.fixture(scope="module")
def selections():
    return {name: run_search(*case) for name, case in cv.selection_cases().items()}


def test_score_never_decreases_along_a_search(selections):
    seen_moves = False
    for name, rep in selections.items():
        best = [s["scores"][s["chosen"]] for s in rep["scans"]]
        assert all(b >= a for a, b in zip(best, best[1:])), (name, best)
        assert rep["score"] == best[-1]
        nobs, o = cv.selection_cases()[name][1], cv.selection_cases()[name][4]
        assert len(rep["scans"]) == (1 + nobs if o.per_observable else 1)
        seen_moves = seen_moves or len(set(rep["scale"])) > 1
    assert seen_moves          # some coordinate scan moved off the common choice


def test_gap_condition_of_the_selection_cases(selections):
    """For every scan of every search the GPU tests repeat, the best finite score leads the runner-up by at least 1e-9:
    a last-bit difference cannot decide one of those tests."""
    for name, rep in selections.items():
        for s in rep["scans"]:
            g = cv.gap(s["scores"])
            print("%s, observable %d: gap %.3g, chose %g" % (name, s["observable"], g, s["grid"][s["chosen"]]))
            assert g >= 1e-9, (name, s["observable"], g)


def test_subset_case_scores_the_rows_the_rule_names(selections):
    x, nobs, lower, upper, o = cv.selection_cases()["blob_2d_subset"]
    rows, n, _ = cv.scored_rows(x.ravel(), x.shape[1], nobs, lower, upper, o.max_rows)
    assert n > o.max_rows and selections["blob_2d_subset"]["rows_used"] == len(rows) == len(cv.subset(n, o.max_rows))
    assert len(rows) <= o.max_rows


def test_unit_gaussian_chooses_a_multiplier_near_one():
    x, lower, upper = cv.unit_gaussian(21, 1000)
    rep = run_search(x, 1, lower, upper, cv.Options(max_rows=0, per_observable=False))
    print("unit Gaussian, 1000 rows: chose %g, score %.6f, at s = 1 %.6f" % (rep["scale"][0], rep["score"],
                                                                          rep["score_at_one"]))
    assert 0.5 <= rep["scale"][0] <= 2.0 and not rep["at_edge"][0]
    assert rep["score"] >= rep["score_at_one"]


def test_two_peaks_choose_a_small_multiplier_and_score_far_better():
    x, lower, upper = cv.two_peaks(11)
    rep = run_search(x, 1, lower, upper, cv.Options(max_rows=0))
    print("two peaks, 400 rows: chose %g, score %.6f, at s = 1 %.6f" % (rep["scale"][0], rep["score"],
                                                                     rep["score_at_one"]))
    assert rep["scale"][0] < 0.5
    assert rep["score"] - rep["score_at_one"] > 0.5
    assert rep["at_edge"][0] == (rep["scale"][0] in (0.125, 4.0))


# ------------------------------------------------------------------ the host arithmetic
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    out = {}
    src = os.path.join(ROOT, "tests", "cpp", "kde_cv_host.cpp")
    for name, flags in HOST_FLAGS.items():
        exe = str(tmp_path_factory.mktemp("kde_cv_host_" + name) / "kde_cv_host")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, src], check=True,
                       capture_output=True, text=True, timeout=300)
        out[name] = exe
    return out


@pytest.mark.parametrize("build", sorted(HOST_FLAGS))
def test_host_arithmetic_stand_alone(host_programs, build):
    r = subprocess.run([host_programs[build]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "kde_cv_host: ok" in r.stdout, r.stdout + r.stderr


def host(host_programs, *args):
    r = subprocess.run([host_programs["asan-ubsan"]] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_reference_restates_the_header(host_programs):
    for lo, hi, steps in ((0.125, 4.0, 21), (0.25, 4.0, 9), (0.3, 1.7, 5), (0.9, 1.1, 3), (0.7, 0.7, 1), (0.25, 2.0, 7),
                          (0.01, 100.0, 32)):
        got = [float.fromhex(v) for v in host(host_programs, "grid", repr(lo), repr(hi), steps)]
        assert got == list(cv.grid(lo, hi, steps))
    for lo, hi, steps in ((0.125, 4.0, 0), (0.125, 4.0, 33), (0.0, 4.0, 21), (4.0, 0.125, 21)):
        with pytest.raises(ValueError) as e:
            cv.grid(lo, hi, steps)
        assert host(host_programs, "grid", repr(lo), repr(hi), steps) == ["error: " + str(e.value)]
    for K in (1, 3, 21, 32):
        for m in (2, 3, 255, 256, 257, 513, 4096, 4097, 8192, 8193, 65536, 131072):
            assert host(host_programs, "split", m, K) == ["%d %d" % cv.split(m, K)]
    for n, R in ((99, 100), (100, 100), (101, 100), (201, 100), (1000, 0), (7, 3)):
        assert [int(v) for v in host(host_programs, "subset", n, R)] == list(cv.subset(n, R))


# ------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    assert NEW_ENTRY_POINTS <= set(declared_symbols())
    assert NEW_ENTRY_POINTS <= exported(capi.LIB_PATH)
    assert NEW_ENTRY_POINTS <= set(capi.SIGNATURES)


def test_bad_arguments_are_refused_without_a_device():
    lib = capi.load()
    bw, sc = np.ones(2), np.zeros(2)
    m = C.c_size_t(0)
    assert lib.sxmc_kde_cv_scores(None, capi.ptr(bw), 1, 0, capi.ptr(sc), C.byref(m)) == capi.ERR_INVALID
    assert capi.last_error() == "null argument"
    assert lib.sxmc_kde_cv_select(None, 0.125, 4.0, 21, 1, 0, capi.ptr(sc), 2, None, None, None, None, None, None, None,
                                  None) == capi.ERR_INVALID
    assert lib.sxmc_kde_bandwidth_scale(None, capi.ptr(sc), 2) == capi.ERR_INVALID
    assert pdfz.CvOptions() == pdfz.CvOptions(0.125, 4.0, 21, True, 65536)
    assert hasattr(pdfz.EvalKernel, "CrossValidated") and hasattr(pdfz.EvalKernel, "SelectBandwidthScale")
