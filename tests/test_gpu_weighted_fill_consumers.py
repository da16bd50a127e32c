"""GPU: what reads a weighted evaluator's histogram -- Project, ProjectCounts, RandomSample, make_asimov_dataset,
fit_spectra -- gives, as BYTES, what it gives on the evaluator over the table with row i repeated m_i times: every
consumer is linear in the integer counts, and n_mc is the multiplicities' total."""
import numpy as np
import pytest

from sxmc_amd import ensemble
from tests import hist_sample_reference as ref
from tests.test_gpu_weighted_fill_walk import tables, workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair():
    """(weighted workload, its evaluators, repeated-table workload, its evaluators), built once."""
    ww, wr = workload("mult", 900), workload("repeated", 900)
    evw, evr = ensemble.make_evaluators(ww), ensemble.make_evaluators(wr)
    yield ww, evw, wr, evr
    for e in evw + evr:
        e.close()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_n_mc_is_the_multiplicity_total(pair):
    ww, evw, wr, evr = pair
    _, mult = tables()
    assert [s.n_mc for s in ww.signals] == [int(m.sum()) for m in mult] == [s.n_mc for s in wr.signals]
    assert [e.SampleTotal() for e in evw] == [s.n_mc for s in ww.signals]
    assert [e.nsamples for e in evw] == [len(m) for m in mult]          # nsamples stays the row count


def test_projections_and_sampler(pair):
    ww, evw, wr, evr = pair
    means = ww.parameter_means()[ww.nsources:]
    geom = ref.Geometry(ww.lower, ww.upper, ww.nbins)
    for j, (a, b) in enumerate(zip(evw, evr)):
        effa, binsa, na = ensemble.get_efficiency(a, ww.nsyst_pars, means, ww.signals[j].n_mc)
        effb, binsb, nb = ensemble.get_efficiency(b, wr.nsyst_pars, means, wr.signals[j].n_mc)
        assert na == nb and effa == effb and same(binsa, binsb)
        for k in range(ww.nobs):
            assert same(a.ProjectCounts(k), b.ProjectCounts(k))
            assert same(a.Project(k, ww.nbins[k]), b.Project(k, ww.nbins[k]))
        got, twin = a.RandomSample(500, 99 + j), b.RandomSample(500, 99 + j)
        assert same(got, twin)
        want = ref.draw(np.asarray(binsa), geom, 500, 99 + j)            # the sampler's law, fed the weighted bins
        assert want["exhausted"] == 0 and same(got, want["events"])


def test_asimov_dataset(pair):
    ww, evw, wr, evr = pair
    rows_a, weights_a, nexp_a = ensemble.make_asimov_dataset(ww, evw)
    rows_b, weights_b, nexp_b = ensemble.make_asimov_dataset(wr, evr)
    assert rows_a.shape[0] > 0 and same(rows_a, rows_b) and same(weights_a, weights_b) and nexp_a == nexp_b


def test_fit_spectra(pair):
    ww, evw, wr, evr = pair
    params = ww.parameter_means().copy()
    params[0], params[ww.nsources] = 1.25, 0.03
    sa, sb = ensemble.fit_spectra(ww, evw, params, ww.events), ensemble.fit_spectra(wr, evr, params, wr.events)
    assert len(sa) == len(sb) == ww.nobs
    for a, b in zip(sa, sb):
        assert same(a["fit"], b["fit"]) and same(a["data"], b["data"])
        for x, y in zip(a["signals"], b["signals"]):
            assert x["nexp"] == y["nexp"] and x["nexp"] > 0 and same(x["spectrum"], y["spectrum"])
