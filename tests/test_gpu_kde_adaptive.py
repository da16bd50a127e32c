"""GPU tests of pdfz::EvalKernel with adaptive (sample-point) bandwidths against the f64 reference
(tests/kde_adaptive_reference.py, which derives the bound of the adaptive pair kernel's f32 arithmetic):

* the local factors: against the reference at 1e-11 relative on every row (terms that matter have exponent <~ 40, so
  its rounding moves a term by <~ 40 (D + 3) 2^-53 ~ 3e-14; exp and erfc are a few ulp; the ordered sum of n <= 3000
  positive terms adds <~ n 2^-53; together below 1e-12, which 1e-11 leaves a factor 10 above -- and five orders under
  the f32 unit, so the value tests may use the reference's own factors); the same bits from two constructions and from a
  shared evaluator; exactly 1.0 at sensitivity 0;
* sensitivity 0 is the fixed-bandwidth evaluator bit for bit: values, norm, events, projections;
* values in 1-4 D at sensitivity 0.5 and 1 with all four systematic kinds, offsets and strides, split and unsplit pair
  sums, a clip case, rows that move into the domain -- each with negative controls (planted errors the comparison must
  see);
* the sampler by law (KS against the adaptive mixture CDF), by bits and by domain; the projection at 1e-11;
* end to end: a configuration with "bandwidth_sensitivity" through the Python layers and the C++ ensemble."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import ensemble, io, pdfz
from sxmc_amd.mcmc import make_systematic
from tests.kde_adaptive_reference import (ADAPTIVE_PLANTS, adaptive_ks_distance, adaptive_mixture_cdf,
                                          moved_with_factors, ref_adaptive_marginal, ref_kde_adaptive,
                                          ref_local_factors, ref_pilot)
from tests.kde_reference import PLANTS, check_power, check_values, compare, mixture_cdf, ref_bandwidths, ref_transform
from tests.project_reference import U24
from tests.test_gpu_kde import gpu_kde
from tests.test_gpu_kde_dims import case, choose_split, hist_norm, points
from tests.test_kde_sample_cpu import build_cpp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = [0.9, 1.1, 0.8, 1.2]


def adaptive(samples, nf, D, lower, upper, scale, alpha, systs=(), dataset=0):
    ev = pdfz.EvalKernel(samples, nf, D, list(lower), list(upper), scale, dataset=dataset, bandwidth_sensitivity=alpha)
    for s in systs:
        ev.AddSystematic(make_systematic(s))
    return ev


def evaluated(ev, D, lower, upper, systs, params, do_eval_pdf=True):
    """`ev` after an evaluation at `params` (norm and pdf at a few points)."""
    pts = np.zeros((4, D + 1), np.float32)
    pts[:, :D] = (np.asarray(lower) + np.asarray(upper)) / 2
    return gpu_kde(None, None, D, lower, upper, None, systs, params, pts.ravel(), ev=ev, do_eval_pdf=do_eval_pdf)


def all_plants(D):
    return list(ADAPTIVE_PLANTS) + [p for p in PLANTS if p != "swap" or D >= 2]


# ------------------------------------------------------------------ the factors
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_local_factors(D):
    rng = np.random.default_rng(7000 + D)
    samples, nf, lower, upper, systs, _ = case(D, 1, 3000, rng)
    if D == 2:                                   # a row no pilot value exists for: it takes 10
        samples = samples.copy()
        samples[5 * nf] = np.nan
    scale = SCALE[:D]
    want = ref_local_factors(samples, nf, D, lower, upper, scale, 0.5)
    _, inside, _ = ref_pilot(samples, nf, D, lower, upper, scale)
    assert 20 < (~inside).sum() < 1500           # rows outside the domain have factors too
    ev = adaptive(samples, nf, D, lower, upper, scale, 0.5, systs)
    got = ev.LocalFactors()
    assert got.dtype == np.float64 and got.shape == (3000,) and ev.BandwidthSensitivity() == 0.5
    rel = float(np.max(np.abs(got - want) / want))
    print("D=%d: lambda %.3g .. %.3g, worst relative error %.3g" % (D, got.min(), got.max(), rel))
    assert rel <= 1e-11
    if D == 2:
        assert got[5] == 10.0
    assert got.min() < 0.9 and got.max() > 1.5   # (the table spreads them: the comparison is not of ones)
    again = adaptive(samples, nf, D, lower, upper, scale, 0.5, systs)
    assert again.LocalFactors().tobytes() == got.tobytes()
    shared = pdfz.EvalKernel.Shared(ev)
    assert shared.LocalFactors().tobytes() == got.tobytes() and shared.BandwidthSensitivity() == 0.5
    ev.close()                                   # the shared evaluator keeps its copy
    assert shared.LocalFactors().tobytes() == got.tobytes()
    # another sensitivity, other factors; sensitivity 0: exactly 1.0, from either constructor
    one = adaptive(samples, nf, D, lower, upper, scale, 1.0)
    assert np.max(np.abs(one.LocalFactors() - ref_local_factors(samples, nf, D, lower, upper, scale, 1.0))
                  / one.LocalFactors()) <= 1e-11
    zero = adaptive(samples, nf, D, lower, upper, scale, 0.0)
    old = pdfz.EvalKernel(samples, nf, D, list(lower), list(upper), scale)
    for e in (zero, old):
        assert np.all(e.LocalFactors() == 1.0) and e.BandwidthSensitivity() == 0.0
    for e in (again, shared, one, zero, old):
        e.close()


# ------------------------------------------------------------------ sensitivity 0 is the evaluator as it was
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_sensitivity_zero_is_the_fixed_evaluator_bit_for_bit(D):
    rng = np.random.default_rng(7100 + D)
    samples, nf, lower, upper, systs, params = case(D, 1, 3000, rng)
    pts = points(D, lower, upper, 600, rng)
    scale = SCALE[:D]
    old = gpu_kde(samples, nf, D, lower, upper, scale, systs, params, pts)
    new = gpu_kde(None, None, D, lower, upper, None, systs, params, pts,
                  ev=adaptive(samples, nf, D, lower, upper, scale, 0.0, systs))
    assert new["norm"] == old["norm"] and new["values"].tobytes() == old["values"].tobytes()
    assert new["ev"].RandomSample(20000, 11).tobytes() == old["ev"].RandomSample(20000, 11).tobytes()
    for obs in range(D):
        assert new["ev"].Project(obs, 65).tobytes() == old["ev"].Project(obs, 65).tobytes()
    # and the adaptive evaluator is another PDF on the same inputs (the identity above is not vacuous)
    ad = gpu_kde(None, None, D, lower, upper, None, systs, params, pts,
                 ev=adaptive(samples, nf, D, lower, upper, scale, 0.5, systs))
    assert ad["norm"] == old["norm"] and ad["values"].tobytes() != old["values"].tobytes()
    for r in (old, new, ad):
        r["ev"].close()


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("D,extra", [(1, 1), (2, 1), (3, 2), (4, 3)], ids=["D1", "D2", "D3", "D4"])
def test_values(D, extra, alpha):
    """3000 samples (no multiple of the 256-row tile) and 600 points: choose_split cuts the tiles over workgroups."""
    rng = np.random.default_rng(7200 + 10 * D + int(2 * alpha))
    samples, nf, lower, upper, systs, params = case(D, extra, 3000, rng)
    pts = points(D, lower, upper, 600, rng)
    scale = SCALE[:D]
    assert choose_split(768, 12)[0] > 1
    args = (samples, nf, D, lower, upper, scale, alpha, systs, params, pts)
    ref = ref_kde_adaptive(*args)
    got = gpu_kde(None, None, D, lower, upper, None, systs, params, pts, par_off=3, par_stride=2, pdf_off=5,
                  pdf_stride=3, norm_off=1, ev=adaptive(samples, nf, D, lower, upper, scale, alpha, systs))
    assert got["norm"] == ref.norm == hist_norm(samples, nf, D, lower, upper, systs, params, 3, 2)
    assert 2000 < ref.norm < 3000
    raw = got["raw"]
    assert np.all(raw[:5] == 12345.0) and np.all(raw[6::3] == 12345.0) and np.all(raw[7::3] == 12345.0)
    label = "D=%d alpha=%g" % (D, alpha)
    check_values(got["values"], ref, label)
    check_power(got["values"], lambda p: ref_kde_adaptive(*args, plant=p), all_plants(D), label)
    got["ev"].close()


@pytest.mark.parametrize("D", [2, 3])
def test_values_unsplit_pair_sum(D):
    """2048 point blocks over two tiles: choose_split keeps the tiles in one workgroup; every 64th point compared."""
    rng = np.random.default_rng(7300 + D)
    samples, nf, lower, upper, systs, params = case(D, 1, 400, rng)
    npts = 2048 * 256 - 100
    assert choose_split(2048 * 256, 2) == (1, 2)
    pts = points(D, lower, upper, npts, rng, other=0.0, outside=0.0)
    got = gpu_kde(None, None, D, lower, upper, None, systs, params, pts,
                  ev=adaptive(samples, nf, D, lower, upper, [1.0] * D, 1.0, systs))
    sub = pts.reshape(npts, D + 1)[::64]
    args = (samples, nf, D, lower, upper, [1.0] * D, 1.0, systs, params, sub.ravel())
    ref = ref_kde_adaptive(*args)
    assert got["norm"] == ref.norm
    check_values(got["values"][::64], ref, "unsplit D=%d" % D)
    check_power(got["values"][::64], lambda p: ref_kde_adaptive(*args, plant=p), all_plants(D), "unsplit D=%d" % D)
    got["ev"].close()


def clip_table():
    """A narrow line on a broad bump on a flat floor: at sensitivity 1 the line's rows clip at 0.1, the floor's at 10."""
    rng = np.random.default_rng(9)
    lower, wid = np.array([-1.0, 0.0]), np.array([4.0, 1.5])
    upper, mid = lower + wid, lower + wid / 2
    x = np.concatenate([mid + 0.004 * wid * rng.normal(size=(600, 2)), mid + 0.12 * wid * rng.normal(size=(2100, 2)),
                        rng.uniform(lower, upper, (300, 2))])
    return x.astype(np.float32).ravel(), lower, upper, rng


def test_values_where_the_factors_clip():
    samples, lower, upper, rng = clip_table()
    D, scale, alpha = 2, [0.3, 0.3], 1.0
    lam = ref_local_factors(samples, D, D, lower, upper, scale, alpha)
    _, inside, _ = ref_pilot(samples, D, D, lower, upper, scale)
    low, high = np.mean(lam[inside] == 0.1), np.mean(lam[inside] == 10.0)
    print("in-domain rows at lambda 0.1: %.1f %%, at 10: %.1f %%, between: %.1f %%"
          % (100 * low, 100 * high, 100 * (1 - low - high)))
    assert low >= 0.01 and high >= 0.01 and 1 - low - high >= 0.5
    systs, params = [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=1, pars=[1])], {0: 0.01, 1: -0.004}
    pts = points(D, lower, upper, 600, rng)
    # and points on the line, where the narrowest kernels and the largest 1 / lambda^2 decide the value
    mid = (lower + upper) / 2
    on = np.zeros((64, 3), np.float32)
    on[:, :2] = mid + 0.004 * (upper - lower) * rng.normal(size=(64, 2))
    pts = np.concatenate([pts, on.ravel()])
    ev = adaptive(samples, D, D, lower, upper, scale, alpha, systs)
    assert float(np.max(np.abs(ev.LocalFactors() - lam) / lam)) <= 1e-11
    args = (samples, D, D, lower, upper, scale, alpha, systs, params, pts)
    ref = ref_kde_adaptive(*args)
    got = gpu_kde(None, None, D, lower, upper, None, systs, params, pts, ev=ev)
    assert got["norm"] == ref.norm
    check_values(got["values"], ref, "clips")
    check_power(got["values"], lambda p: ref_kde_adaptive(*args, plant=p), ["unclipped"] + all_plants(D), "clips")
    ev.close()


def test_rows_that_move_into_the_domain_keep_their_factors():
    rng = np.random.default_rng(7400)
    D = 2
    lower, upper = np.array([0.0, -1.0]), np.array([4.0, 1.0])
    x = np.stack([rng.normal(2.0, 0.7, 3000), rng.uniform(-1, 1, 3000)], axis=1)
    x[:300, 0] = rng.uniform(4.0, 4.6, 300)               # start outside, up to 2 bandwidths and more beyond upper
    samples = x.astype(np.float32).ravel()
    systs, params = [dict(type="shift", obs=0, pars=[0])], {0: -0.7}
    scale, alpha = [1.0, 1.0], 0.5
    lam = ref_local_factors(samples, D, D, lower, upper, scale, alpha)
    _, inside0, _ = ref_pilot(samples, D, D, lower, upper, scale)
    s = ref_transform(samples, D, systs, params)[:, :D]
    inside1 = np.all((s >= lower) & (s < upper), axis=1)
    came = ~inside0 & inside1
    assert came[:300].sum() >= 290 and np.any(lam[came] == 10.0) and np.any(lam[came] < 10.0)
    pts = points(D, lower, upper, 600, rng, outside=0.0)
    pts.reshape(-1, 3)[:200, 0] = rng.uniform(3.2, 3.95, 200).astype(np.float32)     # where the moved-in rows land
    args = (samples, D, D, lower, upper, scale, alpha, systs, params, pts)
    ref = ref_kde_adaptive(*args)
    ev = adaptive(samples, D, D, lower, upper, scale, alpha, systs)
    got = gpu_kde(None, None, D, lower, upper, None, systs, params, pts, ev=ev)
    assert got["norm"] == ref.norm == int(inside1.sum())
    check_values(got["values"], ref, "moved in")
    check_power(got["values"], lambda p: ref_kde_adaptive(*args, plant=p), all_plants(D), "moved in")
    ev.close()


# ------------------------------------------------------------------ the sampler
def test_sampler_law_1d():
    rng = np.random.default_rng(7500)
    lo, hi = 0.0, 10.0
    x = np.concatenate([np.clip(rng.normal(5.0, 0.25, 1500), 2.0, 8.0), rng.uniform(0.0, 10.0, 2000),
                        rng.uniform(0.0, 0.6, 298), rng.uniform(9.4, 10.0, 298)]).astype(np.float32)
    assert x.size == 4096
    alpha = 1.0
    ev = adaptive(x, 1, 1, [lo], [hi], [1.0], alpha)
    got = evaluated(ev, 1, [lo], [hi], [], {})
    s, lam = moved_with_factors(x, 1, 1, [lo], [hi], [1.0], alpha, [], {})
    assert ev.SamplePool() == got["norm"] == len(s) == 4096 and lam.min() < 0.5 and lam.max() > 2
    h = float(ref_bandwidths(x, 1, 1, np.array([lo]), np.array([hi]), [1.0])[0])
    N = 200000
    events = ev.RandomSample(N, 12345)
    xs = events[:, 0].astype(np.float64)
    assert np.all((xs >= lo) & (xs < hi)) and np.all(events[:, 1] == 0.0)
    d = adaptive_ks_distance(xs, s[:, 0], h * lam, lo, hi) * math.sqrt(N)
    print("KS D sqrt(N) = %.4f" % d)
    assert d < 1.95
    # power: the fixed-bandwidth law is another one, at this N
    grid = np.linspace(lo, hi, 4001)
    assert np.max(np.abs(adaptive_mixture_cdf(grid, s[:, 0], h * lam, lo, hi)
                         - mixture_cdf(grid, s[:, 0], h, lo, hi))) * math.sqrt(N) > 1.95
    ev.close()


def test_sampler_law_4d_bits_domain_and_cuts():
    rng = np.random.default_rng(7600)
    D, alpha = 4, 0.5
    samples, nf, lower, upper, systs, params = case(D, 3, 2000, rng)
    scale = [1.2, 0.9, 1.0, 1.5]
    ev = adaptive(samples, nf, D, lower, upper, scale, alpha, systs)
    got = evaluated(ev, D, lower, upper, systs, params)
    s, lam = moved_with_factors(samples, nf, D, lower, upper, scale, alpha, systs, params)
    assert ev.SamplePool() == got["norm"] == len(s)
    h = ev.Bandwidths()
    N = 100000
    events = ev.RandomSample(N, 2024)
    x = events[:, :D].astype(np.float64)
    assert np.all((x >= lower) & (x < upper)) and np.all(events[:, D] == 0.0)
    for d in range(D):
        ks = adaptive_ks_distance(x[:, d], s[:, d], h[d] * lam, lower[d], upper[d]) * math.sqrt(N)
        print("4-D marginal %d: KS D sqrt(N) = %.3f" % (d, ks))
        assert ks < 1.95
    # the same seed, the same bits -- on a shared evaluator too; another seed, other events
    assert ev.RandomSample(N, 2024).tobytes() == events.tobytes()
    assert np.mean(ev.RandomSample(N, 2025)[:, 0] != events[:, 0]) > 0.99
    shared = pdfz.EvalKernel.Shared(ev)
    sh = evaluated(shared, D, lower, upper, systs, params)
    assert sh["norm"] == got["norm"] and sh["values"].tobytes() == got["values"].tobytes()
    assert shared.RandomSample(N, 2024).tobytes() == events.tobytes()
    # cuts redraw: every event inside them, inclusive
    lo = (lower + 0.3 * (upper - lower)).astype(np.float32)
    hi = (lower + 0.6 * (upper - lower)).astype(np.float32)
    c = ev.RandomSample(50000, 8, lowers=lo, uppers=hi)[:, :D]
    assert np.all((c >= lo) & (c <= hi)) and np.all(c.std(axis=0) > 0.02 * (upper - lower))
    shared.close()
    ev.close()


# ------------------------------------------------------------------ the projection
@pytest.mark.parametrize("N", [255, 257, 1000])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_projection(D, N):
    rng = np.random.default_rng(7700 + 10 * D + N)
    samples, nf, lower, upper, systs, params = case(D, 1, N, rng)
    scale, alpha = SCALE[:D], 1.0
    ev = adaptive(samples, nf, D, lower, upper, scale, alpha, systs)
    evaluated(ev, D, lower, upper, systs, params, do_eval_pdf=False)
    args = (samples, nf, D, lower, upper, scale, alpha, systs, params)
    for obs in range(D):
        for nb in (1, 64, 65):
            got = ev.Project(obs, nb)
            assert got.dtype == np.float64 and got.shape == (nb,)
            want, _, _, _ = ref_adaptive_marginal(*args, obs, nb)
            exact, u_max, mass_min, lam_min = ref_adaptive_marginal(*args, obs, nb, rounded=False)
            d, dx = float(np.abs(got - want).max()), float(np.abs(got - exact).max())
            tol_exact = 0.4 * u_max * U24 / mass_min / lam_min
            print("D=%d N=%d obs %d nbins %d: |d| %.3g (rows) %.3g (exact, tolerance %.3g), sum - 1 %.3g"
                  % (D, N, obs, nb, d, dx, tol_exact, got.sum() - 1.0))
            assert d <= 1e-11
            assert dx <= tol_exact
            assert abs(got.sum() - 1.0) <= 1e-11
            assert ev.Project(obs, nb).tobytes() == got.tobytes()
            if nb > 1:                                     # power: every factor 1 % off, or all ones, shows
                assert float(np.abs(got - ref_adaptive_marginal(*args, obs, nb, factor_scale=1.01)[0]).max()) > 1e-11
                fixed = ref_adaptive_marginal(samples, nf, D, lower, upper, scale, 0.0, systs, params, obs, nb)[0]
                assert float(np.abs(got - fixed).max()) > 1e-11
    ev.close()


# ------------------------------------------------------------------ end to end
STEPS, EXPERIMENTS = 200, 2


def write_config(tmp_path, sensitivity):
    rng = np.random.default_rng(27)
    n1, n2 = 20000, 2000
    t1 = 10 * rng.random(n1) * rng.random(n1)
    t2 = np.concatenate([rng.normal(6.0, 0.15, n2 // 2), rng.normal(6.0, 0.9, n2 - n2 // 2)])
    io.write_table(tmp_path / "spectrum.npz", np.stack([t1 + rng.normal(0, 0.2, n1), t1], axis=1), ["e", "e_true"])
    io.write_table(tmp_path / "line.npz", np.stack([t2 + rng.normal(0, 0.1, n2), t2], axis=1), ["e", "e_true"])
    line = {"filename": "line.npz", "dataset": 0, "rate": 300.0, "systematics": ["e_scale"], "pdf": "kernel",
            "bandwidth_scale": 1.0}
    if sensitivity is not None:
        line["bandwidth_sensitivity"] = sensitivity
    cfg = {
        "fit": {"nexperiments": EXPERIMENTS, "nsteps": STEPS, "seed": 31, "burnin_fraction": 0.2,
                "signals": ["spectrum", "line"], "observables": ["energy"], "signal_name": "line"},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 25, "min": 0.0, "max": 10.0}},
                 "systematics": {"e_scale": {"type": "scale", "observable_field": "e", "mean": [0.0],
                                             "sigma": [0.02]}}},
        "signals": {"spectrum": {"filename": "spectrum.npz", "dataset": 0, "rate": 600.0, "systematics": ["e_scale"]},
                    "line": line}}
    path = tmp_path / ("fit_%s.json" % sensitivity)
    path.write_text(json.dumps(cfg))
    return path


def test_a_configuration_with_an_adaptive_signal_end_to_end(tmp_path):
    """The same configuration through the Python layers (load_config, build_workload, make_evaluators,
    make_fake_dataset, fit_spectra, write_fit_spectra) and through the C++ ones (load_config, build_pdfz,
    ensemble_concurrent with two lanes): the two evaluators agree bit for bit, the chains are finite, and the fake data
    are the adaptive PDF's."""
    path = write_config(tmp_path, 0.5)
    w = io.build_workload(io.load_config(str(path)))
    assert [s.bandwidth_sensitivity for s in w.signals] == [0.0, 0.5]
    evs = ensemble.make_evaluators(w)
    line = evs[1]
    assert isinstance(line, pdfz.EvalKernel) and line.BandwidthSensitivity() == 0.5
    lam = line.LocalFactors()
    assert lam.min() < 0.9 and lam.max() > 1.5
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(0, 10, 500), np.zeros(500)], axis=1).astype(np.float32)
    (tmp_path / "points.f32").write_bytes(pts.tobytes())
    py = gpu_kde(None, None, 1, [0.0], [10.0], None, [], {q: 0.01 for q in range(16)}, pts.ravel(), ev=line)

    exe = build_cpp(tmp_path, "kde_adaptive_fit")
    r = subprocess.run([exe, str(path), str(tmp_path / "points.f32"), "0.01", str(tmp_path / "values.f32"),
                        str(tmp_path / "factors.f64")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["sensitivity"] == 0.5 and out["experiments"] == EXPERIMENTS and out["finite"] and out["accepted"] > 0
    assert out["norm"] == py["norm"] and out["nfactors"] == lam.size
    assert (tmp_path / "factors.f64").read_bytes() == lam.tobytes()
    assert (tmp_path / "values.f32").read_bytes() == py["values"].tobytes()

    # fake data: the histogram signal's rows are unchanged, the kernel signal's are another draw than at sensitivity 0
    w0 = io.build_workload(io.load_config(str(write_config(tmp_path, None))))
    evs0 = ensemble.make_evaluators(w0)
    assert evs0[1].BandwidthSensitivity() == 0.0
    rows, observed = ensemble.make_fake_dataset(np.random.default_rng(9), w, evs)
    rows0, observed0 = ensemble.make_fake_dataset(np.random.default_rng(9), w0, evs0)
    assert list(observed) == list(observed0) and observed[1] > 100
    n0 = observed[0]
    assert rows[:n0].tobytes() == rows0[:n0].tobytes() and np.mean(rows[n0:, 0] != rows0[n0:, 0]) > 0.9

    # the fit spectra at the means: the kernel signal's is nexp times the adaptive marginal
    means = np.concatenate([np.ones(w.nsources), np.zeros(w.nparameters - w.nsources)])
    spectra = ensemble.fit_spectra(w, evs, means, rows)
    io.write_fit_spectra(str(tmp_path / "spectra"), spectra)
    assert os.listdir(tmp_path / "spectra") == ["energy_0.json"]
    sig = spectra[0]["signals"][1]
    s = w.signals[1]
    want = ref_adaptive_marginal(s.samples.ravel(), s.nfields, 1, [0.0], [10.0], [1.0], 0.5, w.systematics,
                                 {0: 0.0}, 0, 25)[0]
    assert sig["nexp"] > 0 and np.max(np.abs(np.asarray(sig["spectrum"]) / sig["nexp"] - want)) <= 1e-11
    for e in evs + evs0:
        e.close()


def test_bench_cpp_runs_a_configuration_with_an_adaptive_signal(tmp_path):
    path = write_config(tmp_path, 0.5)
    exe = os.path.join(ROOT, "tests", "cpp", "bench_cpp")
    r = subprocess.run([exe, "--config", str(path), "--devices", "1"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ensemble_multi_gpu" in r.stdout


def test_python_reference_and_device_agree_on_what_adaptivity_buys():
    """A line on a continuum, 1-D: at the line's centre the adaptive estimate is higher than the fixed one (the peak is
    not smoothed away) -- the reason the feature exists, on the device's own numbers."""
    rng = np.random.default_rng(7800)
    x = np.concatenate([rng.normal(5.0, 0.05, 600), rng.uniform(0, 10, 2400)]).astype(np.float32)
    pts = np.array([[5.0, 0.0]], np.float32).ravel()
    fixed = gpu_kde(x, 1, 1, [0.0], [10.0], [1.0], [], {}, pts)
    ad = gpu_kde(None, None, 1, [0.0], [10.0], None, [], {}, pts, ev=adaptive(x, 1, 1, [0.0], [10.0], [1.0], 1.0))
    assert ad["values"][0] > 1.5 * fixed["values"][0]
    ok, _, _ = compare(ad["values"], ref_kde_adaptive(x, 1, 1, [0.0], [10.0], [1.0], 1.0, [], {}, pts))
    assert ok
    fixed["ev"].close()
    ad["ev"].close()
