"""GPU: the histogram event sampler (sxmc_hist_random_sample, random_sample_kernel) through pdfz.EvalHist.

* Bit for bit against the numpy replica (tests/hist_sample_reference.py): 1-D, 2-D and 3-D histograms filled by a real
  evaluation with systematics -- alone, and as members of an EvalGroup in the ordered and in the boxed form --, event
  counts around the block size and beyond the grid (the grid-stride loop), four seeds, histogram shapes that catch
  searches and unravels going wrong, cuts (through bins, leaving one bin, leaving 1/60 and 1/500 of the content, leaving
  nothing), domains far from zero.
* Every event keeps its bin: the oracle's set_eval_points on the drawn events returns the bin the replica says was
  drawn, never -1, never an empty bin.  No geometry here has a bin without a float32 (asserted: share 0).
* The law, from the events alone (hist_sample_reference.law_report: chi-squares of the bins, of the positions inside
  bins per observable, jointly and bin by bin; under cuts the conditional law), p > 1e-4 by the Wilson-Hilferty
  approximation of tests/test_gpu_kde_sample.py.  The seeds are fixed, and because the device stream equals the
  replica's, every one of these assertions was decided on the CPU beforehand by tests/test_hist_sample_reference_cpu.py
  with the same cases and seeds; that file also shows that the checks fail on five wrong samplers.
* State: the "not filled" error after a sparse look-up and after a consuming step, recovery by EvalAsync(False), shared
  evaluators, zero events, four observables.
* C++ (EvalHist::SampleEvents, tests/cpp/hist_sample_dump.cpp) and Python draw the same bytes.
* make_fake_dataset over a config-3-shaped workload with its energy axis at [30000, 30010).

How many events left their bin or the domain before the float step: test_domains_far_from_zero's docstring."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, ensemble, nll, pdfz, workloads
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import MCMC, make_systematic
from tests import hist_sample_reference as R
from tests.test_gpu_kde_sample import wilson_hilferty_sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def new_evaluator(case, norms=None, slot=0, pbuf=None):
    g = case.geom
    ev = pdfz.EvalHist(case.table, case.nfields, g.nobs, g.lower, g.upper, g.nbins.astype(np.int32),
                       dataset=case.dataset)
    for s in case.systs:
        ev.AddSystematic(make_systematic(s))
    norms = norms if norms is not None else DeviceArray.zeros(1, np.uint32)
    pbuf = pbuf if pbuf is not None else DeviceArray(np.asarray(case.params, np.float64))
    ev.SetNormalizationBuffer(norms, slot)
    ev.SetParameterBuffer(pbuf, 0, 1)
    return ev


def evaluated(case):
    """The case's evaluator after a fill (EvalAsync(False)); its histogram is the oracle's."""
    ev = new_evaluator(case)
    ev.EvalAsync(False)
    ev.EvalFinished()
    bins = ev.GetBins()
    assert np.array_equal(bins, case.oracle_bins())
    return ev, bins


def oracle_lookup(case, events):
    g = case.geom
    return oracle.set_eval_points(oracle.HistGeometry(g.lower, g.upper, [int(b) for b in g.nbins]), events,
                                  case.dataset)


def check_draw(ev, case, bins, n, seed, cuts=None):
    """One draw: the replica's bytes, and every event in the bin that was drawn."""
    lo, hi = cuts if cuts else (None, None)
    got = ev.RandomSample(n, seed, lowers=lo, uppers=hi)
    rep = R.draw(bins, case.geom, n, seed, lo, hi, dataset=case.dataset)
    assert rep["exhausted"] == 0
    assert got.shape == (n, case.geom.nobs + 1) and got.dtype == np.float32
    same = got.tobytes() == rep["events"].tobytes()
    if not same:
        differ = np.flatnonzero(np.any(got.view(np.uint32) != rep["events"].view(np.uint32), axis=1))
        print("%s n=%d seed=%d: %d rows differ, first %d: %s vs %s"
              % (case.name, n, seed, differ.size, differ[0], got[differ[0]], rep["events"][differ[0]]))
    rb = oracle_lookup(case, got)
    other = int(((rb != rep["flat"]) & (rb >= 0)).sum())
    outside = int((rb < 0).sum())
    print("%s n=%d seed=%d: %d events in another bin, %d outside the domain" % (case.name, n, seed, other, outside))
    assert same
    assert rep["nofloat"].sum() == 0                      # no bin without a float32 in these geometries
    assert other == 0 and outside == 0 and np.array_equal(rb, rep["flat"])
    assert np.all(bins[rb] > 0)
    return got, rep, rb


def law(case, bins, events, cuts=None):
    lo, hi = cuts if cuts else (None, None)
    rep = R.law_report(events, oracle_lookup(case, events), bins, case.geom, lo, hi, sf=wilson_hilferty_sf)
    assert all(rep.values()), rep


# ------------------------------------------------------------------------------------ bit for bit, alone
@pytest.mark.parametrize("make", [R.case_1d, R.case_2d, R.case_3d], ids=["1d", "2d", "3d"])
def test_counts_and_seeds_alone(make):
    case = make()
    ev, bins = evaluated(case)
    for n in R.COUNTS:
        for seed in R.SEEDS:
            check_draw(ev, case, bins, n, seed)
    check_draw(ev, case, bins, R.BIG_COUNT, R.SEEDS[3])
    assert ev.RandomSample(0, 5).shape == (0, case.geom.nobs + 1)


@pytest.mark.parametrize("form", ["ordered", "boxed"])
def test_members_of_a_group(form):
    """The histogram of the last evaluation is the group's, in the forms the bench runs."""
    cases = [R.case_3d(300000, 103), R.case_3d(123457, 106)]
    norms = DeviceArray.zeros(2, np.uint32)
    pbuf = DeviceArray(np.asarray(R.C3_PARAMS, np.float64))
    evs = [new_evaluator(c, norms, j, pbuf) for j, c in enumerate(cases)]
    group = nll.EvalGroup(evs)
    if form == "ordered":
        group.SetBoxes(False)
        group.SetOrdering(True, force=True)
    else:
        group.SetBoxes(True)
    assert form in group.LaunchInfo(), group.LaunchInfo()
    group.EvalAsync(False)
    group.EvalFinished()
    for case, ev in zip(cases, evs):
        bins = ev.GetBins()
        assert np.array_equal(bins, case.oracle_bins())
        for n, seed in ((1, R.SEEDS[0]), (256, R.SEEDS[1]), (257, R.SEEDS[2]), (2 ** 16 + 1, R.SEEDS[3])):
            check_draw(ev, case, bins, n, seed)
    # new parameters: the events are those of the new histogram
    pbuf.set(np.asarray([-0.05, 0.01, -0.05], np.float64))
    group.EvalAsync(False)
    group.EvalFinished()
    moved = R.Case("3d", cases[0].geom.lower, cases[0].geom.upper, cases[0].geom.nbins, cases[0].table, R.C3_SYSTS,
                   [-0.05, 0.01, -0.05])
    bins = evs[0].GetBins()
    assert np.array_equal(bins, moved.oracle_bins()) and not np.array_equal(bins, cases[0].oracle_bins())
    check_draw(evs[0], moved, bins, 5000, 3)


# ------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("case", R.shape_cases(), ids=lambda c: c.name)
def test_histogram_shapes(case):
    ev, bins = evaluated(case)
    for n in (1, 257):
        check_draw(ev, case, bins, n, R.SEEDS[3])
    got, rep, rb = check_draw(ev, case, bins, 100000, 21)
    rep = R.law_report(got, rb, bins, case.geom, sf=wilson_hilferty_sf)
    rep.pop("unique", None)          # (one bin of a few floats per axis: rows do repeat)
    assert all(rep.values()), rep


# ------------------------------------------------------------------------------------ cuts
def test_cuts():
    case = R.case_3d()
    ev, bins = evaluated(case)
    for name in ("through_bins", "one_in_sixty", "one_in_500"):
        lo, hi, n, seed = R.CUTS_3D[name]
        got, rep, _ = check_draw(ev, case, bins, n, seed, (lo, hi))
        x = got[:, :3]
        assert np.all((x >= np.asarray(lo, np.float32)) & (x <= np.asarray(hi, np.float32)))
        print("%s: up to %d attempts" % (name, rep["attempts"].max()))
        if name == "one_in_500":
            assert rep["attempts"].max() >= 100          # the redraw path is truly exercised
        if name == "one_in_sixty":
            assert rep["attempts"].max() >= 300
    # 1/500 of the content and many events: some exhaust their 1024 attempts, and the call says how many
    lo, hi, n, seed = R.CUTS_3D["one_in_500_fails"]
    rep = R.draw(bins, case.geom, n, seed, lo, hi)
    assert 0 < rep["exhausted"] < n
    with pytest.raises(capi.SxmcError) as err:
        ev.RandomSample(n, seed, lowers=lo, uppers=hi)
    assert "%d of %d events could not be drawn inside the cuts" % (rep["exhausted"], n) in str(err.value)
    # cuts that leave nothing: the existing message, and the evaluator is usable afterwards
    with pytest.raises(capi.SxmcError) as err:
        ev.RandomSample(100, 5, lowers=[20.0, 2.0, -0.5], uppers=[30.0, 5.0, 0.5])
    assert "100 of 100 events could not be drawn inside the cuts" in str(err.value)
    check_draw(ev, case, bins, 5000, 77)
    # cuts that leave one bin, in 1-D and 2-D
    for make, cuts in ((R.case_1d, R.CUTS_1D["one_bin"]), (R.case_2d, R.CUTS_2D["one_bin"])):
        c = make()
        e, b = evaluated(c)
        lo, hi, n, seed = cuts
        _, rep, rb = check_draw(e, c, b, n, seed, (lo, hi))
        assert np.unique(rb).size == 1


# ------------------------------------------------------------------------------------ far from zero
@pytest.mark.parametrize("name", sorted(R.FAR))
def test_domains_far_from_zero(name):
    """1e6 events per domain, seed FAR_SEED.  Without the float step (the sampler rounding lower + (idx + u) * width to
    f32 and nothing more) this test fails.  The replica without the step -- the arithmetic of the kernel as it was,
    rounded operation by operation as the library is built -- counts, of these 1e6 events, so many that look up into
    another bin / fall outside the domain (tests/test_hist_sample_reference_cpu.py prints them), beside the rate of
    the earlier CPU model with a uniform bin choice:

        [1000, 1001) in 1000 bins       14837 /   29      (model 1.5 % / 3.2e-5)
        [30000, 30010) in 20 bins        1863 /  100      (model 0.19 % / 1.0e-4)
        [1e6, 1e6 + 10) in 20 bins      59525 / 3164      (model 6.0 % / 0.31 %)
        [-250000, -249990) in 20 bins   14850 /  793      (no model figure)

    With the float step both counts are zero."""
    case = R.far_case(name)
    ev, bins = evaluated(case)
    check_draw(ev, case, bins, R.FAR_EVENTS, R.FAR_SEED)


# ------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("name", sorted(R.LAW_CASES))
def test_law(name):
    make, n, seed, cuts = R.LAW_CASES[name]
    case = make()
    ev, bins = evaluated(case)
    lo, hi = cuts if cuts else (None, None)
    got = ev.RandomSample(n, seed, lowers=lo, uppers=hi)
    law(case, bins, got, cuts)
    if name == "3d":
        _, n2, seed2, _ = R.LAW_CASES["3d_other_seed"]
        other = ev.RandomSample(n2, seed2)
        assert R.rows_in_common(got, other, 3) == 0       # two seeds: no row in common


# ------------------------------------------------------------------------------------ state
def test_not_filled_after_a_sparse_lookup_and_shared_evaluators():
    rng = np.random.default_rng(107)
    n = 150001
    tab = np.concatenate([rng.uniform(-0.05, 1.05, (n, 4)), np.zeros((n, 1))], axis=1)
    case = R.Case("sparse", [0.0] * 3, [1.0] * 3, [120, 110, 7], tab,      # 92400 bins: beyond LDS capacity
                  [dict(type="scale", obs=0, pars=[0]), dict(type="resolution_scale", obs=1, true_obs=3, pars=[1, 0])],
                  [0.02, 0.1])
    ev = new_evaluator(case)
    pts = np.concatenate([rng.uniform(0, 1, (3000, 3)), np.zeros((3000, 1))], axis=1).astype(np.float32)
    out = DeviceArray.zeros(3000, np.float32)
    ev.SetEvalPoints(pts)
    ev.SetPDFValueBuffer(out)
    ev.EvalAsync(True)
    ev.EvalFinished()
    with pytest.raises(capi.SxmcError) as err:
        ev.RandomSample(10, 1)
    assert "the histogram is not filled" in str(err.value)
    ev.EvalAsync(False)
    ev.EvalFinished()
    bins = ev.GetBins()
    assert np.array_equal(bins, case.oracle_bins())
    a, _, _ = check_draw(ev, case, bins, 200000, 31)
    # a shared evaluator that has evaluated the same parameters draws the same bytes
    shared = pdfz.EvalHist.Shared(ev)
    norm2 = DeviceArray.zeros(1, np.uint32)
    p2 = DeviceArray(np.asarray(case.params, np.float64))
    shared.SetNormalizationBuffer(norm2)
    shared.SetParameterBuffer(p2)
    shared.EvalAsync(False)
    shared.EvalFinished()
    assert shared.RandomSample(200000, 31).tobytes() == a.tobytes()
    assert shared.RandomSample(0, 31).shape == (0, 4)


def test_not_filled_after_a_consuming_step():
    w = workloads.config3(0.003, nevents=300)
    m = MCMC(w, seed=17, lut_output=False, consume=True, stream=capi.new_stream())
    m.walk(w.events, 20, 0.1, sync_interval=10)
    with pytest.raises(capi.SxmcError) as err:
        m.pdfs[0].RandomSample(10, 1)
    assert "the histogram is not filled" in str(err.value)
    m.group.EvalAsync(False, m.stream)
    m.group.EvalFinished()
    vec = m.proposed_vector.get()
    s = w.signals[0]
    case = R.Case("c3", w.lower, w.upper, w.nbins, s.samples, w.systematics, vec[w.nsources:], s.dataset)
    bins = m.pdfs[0].GetBins()
    assert np.array_equal(bins, case.oracle_bins())
    check_draw(m.pdfs[0], case, bins, 3000, 2)


def test_four_observables_are_refused():
    rng = np.random.default_rng(108)
    tab = np.concatenate([rng.uniform(0, 1, (1000, 4)), np.zeros((1000, 1))], axis=1)
    case = R.Case("4d", [0.0] * 4, [1.0] * 4, [3, 3, 3, 3], tab, [dict(type="shift", obs=0, pars=[0])], [0.01])
    ev = new_evaluator(case)
    ev.EvalAsync(False)
    ev.EvalFinished()
    with pytest.raises(pdfz.Error) as err:
        ev.RandomSample(10, 1)
    assert "Cannot EvalHist::CreateHistogram for dimensions greater than 3!" in str(err.value)


# ------------------------------------------------------------------------------------ C++ and Python
def test_cpp_and_python_draw_the_same_bytes(tmp_path):
    case = [c for c in R.shape_cases() if c.name == "dense"][0]
    ev, bins = evaluated(case)
    exe = os.path.join(ROOT, "tests", "cpp", "hist_sample_dump")
    case.table.tofile(str(tmp_path / "table.f32"))
    g = case.geom
    lists = [",".join(repr(float(v)) for v in g.lower), ",".join(repr(float(v)) for v in g.upper),
             ",".join(str(int(v)) for v in g.nbins)]
    for k, cuts in enumerate((None, ([1.2, 0.9, -0.4], [4.7, 4.1, 0.6]))):
        n, seed = 70001, R.SEEDS[2] - k
        out = tmp_path / ("events%d.f32" % k)
        cmd = [exe, str(tmp_path / "table.f32"), str(case.nfields)] + lists + [repr(case.params[0]), str(seed), str(n),
                                                                             str(out)]
        if cuts:
            cmd += [",".join(repr(v) for v in cuts[0]), ",".join(repr(v) for v in cuts[1])]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "%d events, norm %d" % (n, bins.sum()) in r.stdout, r.stdout + r.stderr
        got, rep, _ = check_draw(ev, case, bins, n, seed, cuts)
        assert out.read_bytes() == got.tobytes() == rep["events"].tobytes()


# ------------------------------------------------------------------------------------ end to end
def test_fake_data_with_the_energy_axis_far_from_zero():
    """Config 3's shape with its energy axis at [30000, 30010) and the samples moved along (the energy scale's width
    shrunk by the same factor, so that a step still moves the energies by a fraction of a bin): every event of every
    signal looks up into a non-empty bin of its own signal, and the first step's NLL is the oracle's."""
    w = workloads.config3(0.003, nevents=100)
    off = 30000.0
    w.lower[0], w.upper[0] = off, off + 10.0
    for s in w.signals:
        t = s.samples.astype(np.float64)
        t[:, 0] += off
        t[:, 3] += off
        s.samples = np.ascontiguousarray(t, np.float32)
    w.events = w.events.copy()
    w.events[:, 0] += np.float32(off)
    w.syst_sigmas = list(np.asarray(w.syst_sigmas, np.float64))
    w.syst_sigmas[1] = w.syst_sigmas[1] * 10.0 / (off + 10.0)
    m = MCMC(w, seed=1)
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    means = w.parameter_means()
    data, observed = ensemble.make_fake_dataset(np.random.default_rng(3), w, m.pdfs, poisson=True)
    at = 0
    for s, n in zip(w.signals, observed):
        ev = data[at:at + n]
        at += n
        bins, _ = oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, means[w.nsources:])
        rb = oracle.set_eval_points(geom, ev, s.dataset)
        assert n > 0 and np.all(rb >= 0) and np.all(bins[rb] > 0)
    assert at == data.shape[0]
    m.setup(data=data, sync_interval=8)
    v = m.proposed_vector.get()
    m.step(debug_mode=True)
    rows, _ = m.flush()
    lut = np.zeros((w.nsignals, data.shape[0]), np.float32)
    norms = np.zeros(w.nsignals, np.uint32)
    for j, s in enumerate(w.signals):
        rbj = oracle.set_eval_points(geom, data, s.dataset)
        bj, nj = oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, v[w.nsources:])
        oracle.eval_pdf(rbj, bj, nj, geom.bin_volume, out=lut[j])
        norms[j] = nj
    want, _ = oracle.full_nll(lut, v, data.shape[0], w.nsignals, w.nsources, w.parameter_means(), w.parameter_sigmas(),
                              [s.nexpected for s in w.signals], [s.n_mc for s in w.signals],
                              [s.source_id for s in w.signals], norms)
    print("NLL %.9g, oracle %.9g" % (rows[0, -1], want))
    assert np.isfinite(want) and abs(rows[0, -1] - np.float32(want)) <= 1e-6 * abs(want)
