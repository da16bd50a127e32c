"""GPU: what reads a kernel-density signal over weighted Monte Carlo samples -- get_efficiency, fit_spectra,
make_fake_dataset -- gives, as BYTES, with every m = 8 and n_mc = 8 n what it gives on the unweighted signal (norm and
n_mc both carry the scale: it cancels exactly), beside a histogram signal; make_evaluators builds such a signal and
refuses the row-count mismatch and the combination with cross-validation by name."""
import numpy as np
import pytest

from sxmc_amd import ensemble, pdfz, workloads

pytestmark = pytest.mark.gpu


def mixed_workload(kind):
    """1-D [0, 10): a flat histogram signal and a narrow kernel-density line (scale + resolution systematics); "plain", or
    "times8": the line's rows all of multiplicity 8."""
    rng = np.random.default_rng(26)
    n1, n2 = 20000, 1023
    t1 = rng.uniform(0, 10, n1)
    t2 = rng.normal(6.0, 0.3, n2)
    flat = np.stack([t1 + rng.normal(0, 0.2, n1), t1, np.zeros(n1)], axis=1).astype(np.float32)
    line = np.stack([t2 + rng.normal(0, 0.2, n2), t2, np.zeros(n2)], axis=1).astype(np.float32)
    sigs = [workloads.Signal(flat, 3, 500.0, 0), workloads.Signal(line, 3, 300.0, 1, pdf="kernel", bandwidth_scale=[0.8])]
    if kind == "times8":
        sigs[1].multiplicities = np.full(n2, 8, np.uint32)
        sigs[1].weight_log2_scale = 3
    systs = [dict(type="scale", obs=0, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=1, pars=[1])]
    ev = np.zeros((400, 2), np.float32)
    ev[:, 0] = np.concatenate([rng.uniform(0, 10, 250), rng.normal(6.0, 0.35, 150)])
    return workloads.Workload("mixed-" + kind, 1, [0.0], [10.0], [20], sigs, systs, [0.01, 0.02], ev, "hist + kernel")


@pytest.fixture(scope="module")
def pair():
    wp, w8 = mixed_workload("plain"), mixed_workload("times8")
    evp, ev8 = ensemble.make_evaluators(wp), ensemble.make_evaluators(w8)
    yield wp, evp, w8, ev8
    for e in evp + ev8:
        e.close()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_make_evaluators_passes_the_multiplicities(pair):
    wp, evp, w8, ev8 = pair
    assert isinstance(ev8[1], pdfz.EvalKernel) and ev8[1].HasSampleMultiplicities() and not evp[1].HasSampleMultiplicities()
    assert w8.signals[1].n_mc == 8 * 1023 == ev8[1].SampleTotal() and ev8[1].nsamples == 1023
    assert same(evp[1].Bandwidths(), ev8[1].Bandwidths())


def test_efficiency_and_fake_data(pair):
    wp, evp, w8, ev8 = pair
    means = wp.parameter_means()[wp.nsources:]
    a = ensemble.get_efficiency(evp[1], wp.nsyst_pars, means, wp.signals[1].n_mc, want_bins=False)
    b = ensemble.get_efficiency(ev8[1], w8.nsyst_pars, means, w8.signals[1].n_mc, want_bins=False)
    assert a[0] == b[0] and 0 < a[0] <= 1 and b[2] == 8 * a[2]
    rows_a, obs_a = ensemble.make_fake_dataset(np.random.default_rng(9), wp, evp)
    rows_b, obs_b = ensemble.make_fake_dataset(np.random.default_rng(9), w8, ev8)
    assert list(obs_a) == list(obs_b) and obs_a[1] > 100 and same(rows_a, rows_b)


def test_fit_spectra(pair):
    wp, evp, w8, ev8 = pair
    params = wp.parameter_means().copy()
    params[1], params[wp.nsources] = 1.25, 0.004
    sa, sb = ensemble.fit_spectra(wp, evp, params, wp.events), ensemble.fit_spectra(w8, ev8, params, w8.events)
    assert len(sa) == len(sb) == 1
    for a, b in zip(sa, sb):
        assert same(a["fit"], b["fit"]) and same(a["data"], b["data"])
        for x, y in zip(a["signals"], b["signals"]):
            assert x["nexp"] == y["nexp"] and x["nexp"] > 0 and same(x["spectrum"], y["spectrum"])


def test_refusals_by_name():
    w = mixed_workload("times8")
    w.signals[1].multiplicities = np.full(1000, 8, np.uint32)
    with pytest.raises(pdfz.Error, match="1000 given for 1023 rows"):
        ensemble.make_evaluators(w)
    w = mixed_workload("times8")
    w.signals[1].bandwidth_cv = dict(steps=5)
    with pytest.raises(pdfz.Error, match="cross-validation of a weighted kernel-density evaluator is not built"):
        ensemble.make_evaluators(w)
