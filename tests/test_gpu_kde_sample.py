"""GPU tests of sampling from pdfz.EvalKernel (sxmc_kde_random_sample) against the law the contract states
(include/sxmc_hip.h): a moved in-domain sample chosen uniformly, then per observable its Gaussian truncated to the
domain -- checked in 1-D (KS against the exact mixture CDF, edge fractions), 2-D with every systematic (chi-square
over a grid of separable truncated CDFs) and 4-D (moments); the domain, cuts, errors, determinism, shared evaluators
(sxmc_kde_create_shared), fake data sets over a mixed workload and the C++ ensemble drivers with a kernel-density
signal.  The numpy restatement of the evaluator is tests/kde_reference.py."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, ensemble, io, pdfz, workloads
from sxmc_amd.capi import DeviceArray
from tests.kde_reference import component_cdf, mixture_cdf, moved_in_domain, phi, ref_bandwidths
from tests.test_gpu_kde import PARAMS_2D, SYSTS_2D, gpu_kde, table_2d
from tests.test_kde_sample_cpu import build_cpp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the law in numpy (f64)
def evaluated(samples, nfields, nobs, lower, upper, scale, systs=(), params=None, dataset=0):
    """An evaluator that has evaluated (norm and pdf at a few points) at `params`."""
    pts = np.zeros((4, nobs + 1), np.float32)
    pts[:, :nobs] = (np.asarray(lower) + np.asarray(upper)) / 2
    pts[:, nobs] = dataset
    return gpu_kde(samples, nfields, nobs, lower, upper, scale, list(systs), params or {}, pts.ravel(),
                   dataset=dataset)


def ks_distance(events, s, h, lo, hi):
    """sup |F_N - F| with F the exact mixture CDF (on a fine grid, linearly interpolated: error far below 1e-5)."""
    grid = np.linspace(lo, hi, 4001)
    F = np.interp(np.sort(events), grid, mixture_cdf(grid, s, h, lo, hi))
    n = len(events)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)))


def edge_fractions_ok(events, s, h, lo, hi):
    """Fraction of events within one bandwidth of each edge against the mixture, within 5 binomial sigma."""
    n = len(events)
    ok = True
    for a, b in ((lo, lo + h), (hi - h, hi)):
        p = float(np.diff(mixture_cdf(np.array([a, b]), s, h, lo, hi))[0])
        got = int(np.sum((events >= a) & (events < b)))
        ok = ok and abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p))
        print("edge [%.4f, %.4f): %d events, mixture %.1f" % (a, b, got, n * p))
    return ok


# ------------------------------------------------------------------ tests
def test_law_1d_truncation_matters():
    rng = np.random.default_rng(21)
    lo, hi = 0.0, 10.0
    x = np.concatenate([np.clip(rng.normal(5.0, 1.2, 2730), 2.0, 8.0),
                        rng.uniform(0.0, 0.6, 683), rng.uniform(9.4, 10.0, 683)]).astype(np.float32)
    assert x.size == 4096
    h = float(ref_bandwidths(x, 1, 1, np.array([lo]), np.array([hi]), [1.0])[0])
    assert np.mean((x < lo + 2 * h) | (x >= hi - 2 * h)) >= 1 / 3
    got = evaluated(x, 1, 1, [lo], [hi], [1.0])
    ev = got["ev"]
    assert np.allclose(ev.Bandwidths(), [h], rtol=1e-12)
    assert ev.SamplePool() == got["norm"] == 4096
    N = 200000
    events = ev.RandomSample(N, 12345)[:, 0].astype(np.float64)
    s = x.astype(np.float64)
    d = ks_distance(events, s, h, lo, hi)
    print("KS D sqrt(N) = %.4f" % (d * math.sqrt(N)))
    assert d * math.sqrt(N) < 1.95
    assert edge_fractions_ok(events, s, h, lo, hi)
    # the check has the power to see a clamped, untruncated Gaussian
    r2 = np.random.default_rng(5)
    wrong = np.clip(s[r2.integers(0, s.size, N)] + h * r2.normal(size=N), lo, np.nextafter(hi, lo))
    assert not (ks_distance(wrong, s, h, lo, hi) * math.sqrt(N) < 1.95 and edge_fractions_ok(wrong, s, h, lo, hi))


def wilson_hilferty_sf(chi2, k):
    z = ((chi2 / k) ** (1.0 / 3.0) - (1 - 2.0 / (9 * k))) / math.sqrt(2.0 / (9 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def test_law_2d_with_all_systematics():
    rng = np.random.default_rng(22)
    samples = table_2d(rng, 4000)
    lower, upper = [0.0, -1.0], [4.0, 1.0]
    got = evaluated(samples, 3, 2, lower, upper, [1.0, 0.7], SYSTS_2D, PARAMS_2D)
    ev = got["ev"]
    s = moved_in_domain(samples, 3, 2, lower, upper, SYSTS_2D, PARAMS_2D)
    assert ev.SamplePool() == got["norm"] == len(s)
    h = ev.Bandwidths()
    N = 400000
    events = ev.RandomSample(N, 777)
    assert np.all(events[:, 2] == 0.0)
    edges = [np.linspace(lower[d], upper[d], 17) for d in range(2)]
    counts, _, _ = np.histogram2d(events[:, 0].astype(np.float64), events[:, 1].astype(np.float64), bins=edges)
    # expected: per sample, the separable truncated CDF differences, summed
    A = [np.diff(component_cdf(edges[d], s[:, d], h[d], lower[d], upper[d]), axis=0) for d in range(2)]   # [16, n]
    expect = N * (A[0] @ A[1].T) / len(s)
    assert abs(expect.sum() - N) < 1e-6 * N
    use = expect >= 5
    chi2 = float((((counts - expect) ** 2) / expect)[use].sum())
    k = int(use.sum()) - 1
    p = wilson_hilferty_sf(chi2, k)
    print("chi2 %.1f over %d dof: p = %.3g" % (chi2, k, p))
    assert p > 1e-4
    assert counts[~use].sum() <= 5 * max(1.0, expect[~use].sum()) + 20


def test_moments_4d():
    rng = np.random.default_rng(23)
    n = 3000
    t = rng.normal(0.0, 1.0, (n, 4)) @ np.array([[1.0, 0.3, 0, 0], [0, 0.8, 0.2, 0], [0, 0, 0.5, 0.1], [0, 0, 0, 0.7]])
    samples = (t + np.array([0.5, 0.0, -0.2, 0.3])).astype(np.float32)
    lower, upper = np.array([-1.5, -2.0, -1.0, -1.0]), np.array([2.0, 2.0, 1.0, 1.5])
    got = evaluated(samples.ravel(), 4, 4, lower, upper, [1.0, 1.5, 0.8, 1.2])
    ev = got["ev"]
    s = moved_in_domain(samples.ravel(), 4, 4, lower, upper, [], {})
    assert ev.SamplePool() == got["norm"] == len(s)
    h = ev.Bandwidths()
    a, b = (lower - s) / h, (upper - s) / h
    pdf = lambda z: np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)   # noqa: E731
    Z = phi(b) - phi(a)
    r = (pdf(a) - pdf(b)) / Z
    m = s + h * r                                                    # per component: truncated means
    v = h * h * (1 + (a * pdf(a) - b * pdf(b)) / Z - r * r)          # ... and variances
    mu = m.mean(axis=0)
    cov = (m.T @ m) / len(s) + np.diag(v.mean(axis=0)) - np.outer(mu, mu)
    N = 200000
    x = ev.RandomSample(N, 4242)[:, :4].astype(np.float64)
    assert np.all((x >= lower) & (x < upper))
    xm = x.mean(axis=0)
    dev = x - xm
    c = dev.T @ dev / N
    se_mean = np.sqrt(np.diag(c) / N)
    se_cov = np.sqrt(np.maximum(((dev[:, :, None] * dev[:, None, :]) ** 2).mean(axis=0) - c * c, 0) / N)
    print("mean pulls", (xm - mu) / se_mean)
    print("max cov pull %.2f" % np.max(np.abs(c - cov) / se_cov))
    assert np.all(np.abs(xm - mu) < 5 * se_mean)
    assert np.all(np.abs(c - cov) < 5 * se_cov)


def test_domain_cuts_errors_and_dataset():
    rng = np.random.default_rng(24)
    # crowded at both edges with a tiny bandwidth; 0.1 is no float: draws round across both bounds unless moved
    lo, hi = 0.1, 0.2
    x = np.concatenate([0.1 + 2e-5 * rng.random(500), 0.2 - 2e-5 * rng.random(500)]).astype(np.float32)
    x = x[(x.astype(np.float64) >= lo) & (x.astype(np.float64) < hi)]
    got = evaluated(x, 1, 1, [lo], [hi], [0.05], dataset=3)
    ev = got["ev"]
    e = ev.RandomSample(100000, 99)
    xs = e[:, 0].astype(np.float64)
    assert np.all(xs >= lo) and np.all(xs < hi)
    top = np.nextafter(np.float32(hi), np.float32(0))
    assert float(top) < hi <= float(np.float32(hi))
    assert np.sum(e[:, 0] == top) > 0                   # events that rounded to `upper` were moved below it
    assert np.all(e[:, 1] == 3.0)                       # the dataset column
    # an upper bound that is a float: the largest float below it
    y = (1.0 - 3e-5 * rng.random(1000)).astype(np.float32)
    ev1 = evaluated(y, 1, 1, [0.0], [1.0], [0.05])["ev"]
    ey = ev1.RandomSample(100000, 5)[:, 0]
    assert np.all(ey < np.float32(1.0)) and np.sum(ey == np.nextafter(np.float32(1), np.float32(0))) > 0
    # cuts, inclusive
    big = evaluated(rng.uniform(0, 10, 3000).astype(np.float32), 1, 1, [0.0], [10.0], [1.0])["ev"]
    c = big.RandomSample(20000, 3, lowers=[2.0], uppers=[3.0])[:, 0]
    assert np.all((c >= 2.0) & (c <= 3.0)) and c.std() > 0.2
    with pytest.raises(capi.SxmcError) as err:
        big.RandomSample(1000, 3, lowers=[20.0], uppers=[30.0])
    assert "1000 of 1000 events" in str(err.value)
    assert big.RandomSample(0, 3).shape == (0, 2)
    # before any evaluation
    fresh = pdfz.EvalKernel(rng.uniform(0, 1, 100).astype(np.float32), 1, 1, [0.0], [1.0], [1.0])
    with pytest.raises(capi.SxmcError) as err:
        fresh.RandomSample(10, 1)
    assert "before an evaluation" in str(err.value)
    # every sample moved out of the domain: nothing to draw from
    gone = gpu_kde(rng.uniform(0.2, 0.8, 200).astype(np.float32), 1, 1, [0.0], [1.0], [1.0],
                   [dict(type="shift", obs=0, pars=[0])], {0: 5.0}, np.zeros(2, np.float32), do_eval_pdf=False)
    assert gone["norm"] == 0 and gone["ev"].SamplePool() == 0
    with pytest.raises(capi.SxmcError) as err:
        gone["ev"].RandomSample(10, 1)
    assert "no sample inside the domain" in str(err.value)


def test_determinism_and_shared_evaluators():
    rng = np.random.default_rng(25)
    samples = table_2d(rng, 20000)
    lower, upper = [0.0, -1.0], [4.0, 1.0]
    pts = np.stack([rng.uniform(0, 4, 3000), rng.uniform(-1, 1, 3000), np.zeros(3000)], axis=1).astype(np.float32)
    base = gpu_kde(samples, 3, 2, lower, upper, [1.0, 1.0], SYSTS_2D, PARAMS_2D, pts.ravel())
    ev = base["ev"]
    a, b = ev.RandomSample(50000, 1), ev.RandomSample(50000, 1)
    assert a.tobytes() == b.tobytes()
    c = ev.RandomSample(50000, 2)
    assert np.mean(c[:, 0] != a[:, 0]) > 0.99
    shared = pdfz.EvalKernel.Shared(ev)
    assert np.array_equal(shared.Bandwidths(), ev.Bandwidths()) and shared.nsamples == ev.nsamples
    sh = gpu_kde(samples, 3, 2, lower, upper, [1.0, 1.0], SYSTS_2D, PARAMS_2D, pts.ravel(), ev=shared)
    assert sh["norm"] == base["norm"] and sh["values"].tobytes() == base["values"].tobytes()
    assert shared.RandomSample(50000, 1).tobytes() == a.tobytes()
    ev.close()                                           # the shared evaluator outlives its base
    del base
    sh2 = gpu_kde(samples, 3, 2, lower, upper, [1.0, 1.0], SYSTS_2D, PARAMS_2D, pts.ravel(), ev=shared)
    assert sh2["norm"] == sh["norm"] and sh2["values"].tobytes() == sh["values"].tobytes()
    assert shared.RandomSample(50000, 1).tobytes() == a.tobytes()
    shared.close()


def mixed_workload(rng):
    """1-D [0, 10): a flat histogram signal and a narrow kernel-density line, scale + resolution systematics."""
    n1, n2 = 100000, 2000
    t1 = rng.uniform(0, 10, n1)
    t2 = rng.normal(6.0, 0.3, n2)
    flat = np.stack([t1 + rng.normal(0, 0.2, n1), t1, np.zeros(n1)], axis=1).astype(np.float32)
    line = np.stack([t2 + rng.normal(0, 0.2, n2), t2, np.zeros(n2)], axis=1).astype(np.float32)
    sigs = [workloads.Signal(flat, 3, 500.0, 0), workloads.Signal(line, 3, 300.0, 1, pdf="kernel",
                                                                  bandwidth_scale=[0.8])]
    systs = [dict(type="scale", obs=0, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=1, pars=[1])]
    return workloads.Workload("mixed", 1, [0.0], [10.0], [20], sigs, systs, [0.01, 0.02],
                              np.zeros((0, 2), np.float32), "hist + kernel")


def test_fake_data_over_a_mixed_workload():
    w = mixed_workload(np.random.default_rng(26))
    evs = ensemble.make_evaluators(w)
    assert isinstance(evs[0], pdfz.EvalHist) and isinstance(evs[1], pdfz.EvalKernel)
    effs = [ensemble.get_efficiency(ev, w.nsyst_pars, w.parameter_means()[w.nsources:], s.n_mc, want_bins=False)[0]
            for s, ev in zip(w.signals, evs)]
    lam = [s.nexpected * e for s, e in zip(w.signals, effs)]
    # one data set replayed draw by draw: each signal's rows are its own evaluator's RandomSample
    rows, observed = ensemble.make_fake_dataset(np.random.default_rng(9), w, evs)
    replay = np.random.default_rng(9)
    at = 0
    for j, ev in enumerate(evs):
        n = int(replay.poisson(lam[j]))
        want = ev.RandomSample(n, int(replay.integers(0, 2 ** 63 - 1)))
        assert n == observed[j] and rows[at:at + n].tobytes() == want.tobytes()
        at += n
    assert at == rows.shape[0]
    line = rows[observed[0]:, 0]
    assert abs(line.mean() - 6.0) < 0.1 and line.std() < 0.6      # the kernel signal's events are the line's
    # the expected Poisson means over many data sets
    K = 200
    rng = np.random.default_rng(10)
    obs = np.array([ensemble.make_fake_dataset(rng, w, evs)[1] for _ in range(K)], np.float64)
    for j in range(2):
        pull = (obs[:, j].mean() - lam[j]) / math.sqrt(lam[j] / K)
        print("signal %d: mean %.2f, expected %.2f (pull %.2f)" % (j, obs[:, j].mean(), lam[j], pull))
        assert abs(pull) < 5
        assert abs(obs[:, j].var(ddof=1) / lam[j] - 1) < 5 * math.sqrt(2.0 / (K - 1))
    for ev in evs:
        ev.close()


STEPS, EXPERIMENTS = 3000, 8


def write_config(tmp_path):
    rng = np.random.default_rng(27)
    n1, n2 = 100000, 3000
    t1 = 10 * rng.random(n1) * rng.random(n1)
    t2 = rng.normal(6.0, 0.4, n2)
    io.write_table(tmp_path / "spectrum.npz", np.stack([t1 + rng.normal(0, 0.2, n1), t1], axis=1), ["e", "e_true"])
    io.write_table(tmp_path / "line.npz", np.stack([t2 + rng.normal(0, 0.2, n2), t2], axis=1), ["e", "e_true"])
    cfg = {
        "fit": {"nexperiments": EXPERIMENTS, "nsteps": STEPS, "seed": 31, "burnin_fraction": 0.2,
                "signals": ["spectrum", "line"], "observables": ["energy"], "signal_name": "line"},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 25, "min": 0.0, "max": 10.0}},
                 "systematics": {"e_scale": {"type": "scale", "observable_field": "e", "mean": [0.0],
                                             "sigma": [0.02]}}},
        "signals": {"spectrum": {"filename": "spectrum.npz", "dataset": 0, "rate": 600.0, "systematics": ["e_scale"]},
                    "line": {"filename": "line.npz", "dataset": 0, "rate": 300.0, "systematics": ["e_scale"],
                             "pdf": "kernel", "bandwidth_scale": 1.0}}}
    path = tmp_path / "fit.json"
    path.write_text(json.dumps(cfg))
    return path


def test_cpp_ensembles_with_a_kernel_signal(tmp_path):
    """ensemble and ensemble_concurrent (2 lanes) agree bit for bit per experiment; ensemble_multi_gpu with default
    options takes the concurrent fallback and agrees too; the kernel signal's mean best-fit rate lies within 3 standard
    errors of the generated one (1.0) over EXPERIMENTS experiments of STEPS steps."""
    path = write_config(tmp_path)
    exe = build_cpp(tmp_path, "kde_ensemble")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["experiments"] == EXPERIMENTS and line["steps"] == STEPS
    assert line["concurrent_identical"] and line["multi_gpu_identical"]
    assert line["lockstep_chains"] >= 2 and line["device_mode"] == "concurrent"
    rate = line["sources"]["line"]
    assert rate["stderr"] > 0 and abs(rate["mean"] - 1.0) < 3 * rate["stderr"], rate


def test_bench_cpp_runs_a_config_with_a_kernel_signal(tmp_path):
    path = write_config(tmp_path)
    exe = os.path.join(ROOT, "tests", "cpp", "bench_cpp")
    r = subprocess.run([exe, "--config", str(path), "--devices", "1"], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ensemble_multi_gpu" in r.stdout
