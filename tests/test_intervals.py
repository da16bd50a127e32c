"""Interval extraction three ways on the SAME chain: the Python form (sxmc_amd/ensemble.py),
the C++ form (sxmc_amd/include/sxmc/intervals.h through tests/cpp/intervals_dump) and the brute-force restatement of
contour.cpp:30-69 / likelihood.cpp:90-102 / projection.cpp:14-77 in oracle/intervals.py -- on synthetic chains here
(CPU) and on a chain walked on the GPU (-m gpu), the printed-offset regime |lmin| ~ 3e5 of BASELINE config 3 included.
Contour intervals must agree bit for bit (they are minima and maxima of chain values once the same rows are
selected); projection limits and coverages exactly, the fitted mean to 1e-6 (three different minimisers of one chi2).
intervals.h needs no device and no library, so the CPU cases run a second time through intervals_dump_asan, the same
program under AddressSanitizer + UndefinedBehaviorSanitizer.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import intervals as ref
from sxmc_amd import ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                 UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def run_dump(exe, args):
    """tests/cpp/<exe> (intervals_dump or intervals_dump_asan), built if need be: its standard output."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), exe])
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", exe)] + args, capture_output=True, text=True, timeout=120,
                       env=SANITIZED)
    assert r.returncode == 0, r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def cpp_intervals(chain, cl, tmp_path, exe="intervals_dump"):
    path = os.path.join(str(tmp_path), "chain.f32")
    np.ascontiguousarray(chain, np.float32).tofile(path)
    out = run_dump(exe, [path, str(chain.shape[1]), repr(float(cl))])
    try:
        return json.loads(out)
    except ValueError:
        raise AssertionError("intervals_dump printed something that is not JSON: " + out[:3000])


def compare_three_ways(chain, cl, tmp_path, exe="intervals_dump"):
    chain = np.ascontiguousarray(chain, np.float32)
    P = chain.shape[1] - 1
    cl32 = float(np.float32(cl))                         # `float cl` in the reference (error_estimator.h)
    cpp = cpp_intervals(chain, cl32, tmp_path, exe)
    py = ensemble.contour_intervals(chain, cl32)
    try:
        want = ref.contour_intervals(chain, cl32)
    except AssertionError:
        # the reference itself stops here (assert at likelihood.cpp:99: with this |lmin| the printed offset is so far
        # off that no row passes).  Product code falls back to the exact offset; Python and C++ must agree on that.
        like = chain[:, -1].astype(np.float64)
        exact = chain[chain[:, -1] - chain[:, -1].min() < np.float32(0.5 * ref.chisquare_quantile_1dof(np.float32(cl32)))]
        want = [(float(py[p, 0]), float(exact[:, p].min()), float(exact[:, p].max()), -999.0) for p in range(P)]
    for p in range(P):
        for k in range(3):                                # point estimate, lower, upper: bit for bit
            assert np.float32(want[p][k]) == py[p, k] == np.float32(cpp["contour"][p][k]), (p, k, want[p], py[p], cpp["contour"][p])
        assert py[p, 3] == -999 and cpp["contour"][p][3] == -999
    for p in range(P):
        w = ref.projection_interval(chain[:, p], cl32)
        a = ensemble.projection_interval(chain[:, p], cl32)
        c = cpp["projection"][p]
        scale = max(abs(w[0]), float(np.ptp(chain[:, p])), 1e-30)
        assert abs(a[0] - w[0]) <= 1e-6 * scale and abs(c[0] - w[0]) <= 2e-6 * scale, (p, w, a, c)    # fitted mean
        assert a[1] == w[1] and a[2] == w[2] and a[3] == w[3] and a[4] == w[4], (p, w, a)             # limits, coverage
        assert np.float32(w[1]) == np.float32(c[1]) and np.float32(w[2]) == np.float32(c[2]), (p, w, c)
        assert abs(c[3] - w[3]) < 1e-6 and c[4] == w[4]
    return want


def synthetic_chain(seed, n, nll_offset, spread=3.0):
    """A Metropolis-looking chain: correlated Gaussian parameters with repeated rows, likelihood = offset + chi2 / 2."""
    rng = np.random.default_rng(seed)
    P = 4
    mean = np.array([1.0, 0.02, -0.5, 250.0])
    sig = np.array([0.1, 0.01, 0.2, 30.0])
    x = mean + sig * rng.standard_normal((n, P))
    x[:, 1] += 0.3 * (x[:, 0] - mean[0]) * sig[1] / sig[0]
    keep = rng.random(n) < 0.4                            # rejected steps repeat the previous row
    for i in range(1, n):
        if not keep[i]:
            x[i] = x[i - 1]
    nll = nll_offset + 0.5 * np.sum(((x - mean) / sig) ** 2, axis=1) * spread / 3.0
    return np.concatenate([x, nll[:, None]], axis=1).astype(np.float32)


@pytest.mark.parametrize("offset", [12.5, -348086.3, 3.2e5, -7.123456e6])
@pytest.mark.parametrize("cl", [0.9, 0.683])
def test_python_cpp_and_restatement_agree_on_synthetic_chains(tmp_path, offset, cl):
    chain = synthetic_chain(int(abs(offset)) % 1000 + int(cl * 100), 4000, offset)
    compare_three_ways(chain, cl, tmp_path)


@pytest.mark.parametrize("offset", [12.5, -348086.3, 3.2e5, -7.123456e6])
@pytest.mark.parametrize("cl", [0.9, 0.683])
def test_synthetic_chains_through_the_sanitizer_build(tmp_path, offset, cl):
    chain = synthetic_chain(int(abs(offset)) % 1000 + int(cl * 100), 4000, offset)
    compare_three_ways(chain, cl, tmp_path, "intervals_dump_asan")


def test_printed_offset_changes_the_contour_at_config3_magnitudes(tmp_path, exe="intervals_dump"):
    """With |lmin| = 348 086.3 the text "likelihood+348086<1.35277" applies an offset that is off by 0.3: the contour
    the reference selects is NOT the exact Delta-NLL contour, and all three implementations follow the reference."""
    chain = synthetic_chain(7, 4000, -348086.3)
    got = compare_three_ways(chain, 0.9, tmp_path, exe)
    like = chain[:, -1].astype(np.float64)
    delta = 0.5 * ref.chisquare_quantile_1dof(np.float32(0.9))
    exact = chain[like - like.min() < delta]
    assert float(got[0][2]) != float(exact[:, 0].max()) or float(got[0][1]) != float(exact[:, 0].min())
    # a one-sided projection: a parameter piled up at its lower bound
    rng = np.random.default_rng(3)
    col = np.abs(rng.standard_normal(5000)).astype(np.float32) * 0.1
    w = ref.projection_interval(col, float(np.float32(0.9)))
    a = ensemble.projection_interval(col, float(np.float32(0.9)))
    assert w[4] is True and a[4] is True and a[1:4] == w[1:4]


def test_printed_offset_through_the_sanitizer_build(tmp_path):
    test_printed_offset_changes_the_contour_at_config3_magnitudes(tmp_path, "intervals_dump_asan")


@pytest.mark.gpu
def test_intervals_of_a_gpu_chain_three_ways(tmp_path):
    """A chain walked on the GPU (BASELINE config 3's shape at 1 % of the samples, 10^5 events: |lmin| of a few 1e5,
    the printed-offset regime) through Contour and Projection in Python and C++, against the restatement."""
    from sxmc_amd import capi, workloads
    from sxmc_amd.mcmc import MCMC
    w = workloads.config3(0.01, nevents=100000)
    for s in w.signals:
        s.nexpected = 100000.0 / w.nsignals               # rates that describe the data: the walk starts near the truth
    m = MCMC(w, seed=11, fused=True, lut_output=False, consume=True, stream=capi.new_stream())
    # long enough for both re-tunings of the proposal (mcmc.cpp:274-311) to take: the kept half samples the posterior
    chain, accepted = m.walk(w.events, 12000, 0.25, sync_interval=1000, graph_steps=8)
    assert chain.shape[0] == 6000 and 300 < accepted < 11000
    assert abs(float(chain[:, -1].min())) > 1e5          # six printed digits cannot hold this offset
    for p in range(w.nparameters):                        # every parameter moved: the projections are real histograms
        assert np.unique(chain[:, p]).size > 50
    compare_three_ways(chain, 0.9, tmp_path)
    compare_three_ways(chain, 0.683, tmp_path)
    for p in m.pdfs:
        p.close()
    m.group.close()


def test_best_fit_and_correlation_report(tmp_path, exe="intervals_dump"):
    """LikelihoodSpace::print_best_fit / print_correlations (likelihood.cpp:34-72, what sxmc.cpp:100-101 prints per
    experiment): the C++ text equals the Python text character for character -- parameters of the best fit in NAME
    order, the matrix' lower triangle zero as the reference leaves it, and the second best-fit block's NLL at the
    precision of 3 that print_correlations leaves on the stream -- and the matrix equals the statement-by-statement loop."""
    rng = np.random.default_rng(11)
    n, names = 700, ["zeta_rate", "alpha", "mid_scale", "b"]
    chain = rng.normal(size=(n, len(names) + 1)).astype(np.float32)
    chain[:, 1] += np.float32(0.7) * chain[:, 0]
    chain[:, 2] = np.float32(3.0) + np.float32(0.01) * chain[:, 2] - np.float32(0.005) * chain[:, 0]
    chain[:, -1] = np.float32(-2.5e5) + np.float32(0.5) * (chain[:, :-1] ** 2).sum(axis=1)
    path = os.path.join(str(tmp_path), "chain.f32")
    chain.tofile(path)
    cl = float(np.float32(0.9))
    out = run_dump(exe, [path, str(chain.shape[1]), repr(cl), "--report", ",".join(names)])
    iv = ensemble.contour_intervals(chain, cl)
    m = ensemble.correlation_matrix(chain)
    want = ensemble.format_best_fit(names, iv, chain[:, -1].min(), cl) + ensemble.format_correlations(names, m) + \
        ensemble.format_best_fit(names, iv, chain[:, -1].min(), cl, precision=3)
    assert out == want, "\n" + out + "\n---\n" + want
    lines = want.splitlines()
    assert [l.split(":")[0].strip() for l in lines[1:5]] == sorted(names)          # std::map order
    assert lines[5].startswith(" NLL: -2499") and lines[-1] == " NLL: -2.5e+05"
    brute = np.asarray(ref.correlation_matrix(chain), np.float32)
    assert np.array_equal(m, brute)
    assert np.all(np.tril(m, -1) == 0) and np.all(np.diag(m) == 1)
    assert abs(m[0, 1] - np.corrcoef(chain[:, 0], chain[:, 1])[0, 1]) < 1e-4
    k = names.index("alpha")
    assert lines[1] == " alpha: " + ref.interval_text(iv[k, 0], iv[k, 1], iv[k, 2])


def test_best_fit_and_correlation_report_through_the_sanitizer_build(tmp_path):
    test_best_fit_and_correlation_report(tmp_path, "intervals_dump_asan")
