"""The Asimov data set (ensemble.make_asimov_dataset) on the device: one observable of 25 bins with two signals, and two
observables of 10 x 6 bins with three; a few thousand samples each, some outside the histogram (efficiencies below 1).

  * its rows look up into the bins they were made from (the oracle's set_eval_points), one row per non-empty bin in flat
    index order, signal by signal;
  * the weights of signal j sum to nexp_j = nexpected_j * eff_j to 1e-12 relative;
  * THE POINT OF IT, with no tolerance: through the group (sxmc_group_eval_nll_async over the weighted classes) and
    nll_total, the NLL of the Asimov data at the nominal rates is strictly below the NLL with any one rate scaled by
    0.9, 0.95, 1.05 or 1.1 -- Gibbs' inequality, exact for histogram signals that share a binning
    (tests/test_asimov_cpu.py checks that at this scale the differences are far above the kernels' 1e-12);
  * a fit of it (ensemble.run_experiment(data=..., event_weights=...)) walks, and no row of its chain lies below that
    minimum.
"""
import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, ensemble, nll, workloads
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import MCMC, REDUCE_THREADS
from tests.test_gpu_step_end_arith import close

pytestmark = pytest.mark.gpu

FIXTURES = {"1 x 25, two signals": (1, [25], 2), "10 x 6, three signals": (2, [10, 6], 3)}


def fixture(name):
    nobs, nbins, nsig = FIXTURES[name]
    rng = np.random.default_rng(40 + nsig)
    lower, upper = [0.0] * nobs, [10.0, 6.0][:nobs]
    signals = []
    for j in range(nsig):
        n = 3000 + 500 * j
        cols = [rng.normal(3.0 + 2.0 * j, 1.5 + 0.5 * j, n)]                 # (tails leave [0, 10): eff < 1)
        if nobs == 2:
            cols.append(6.5 * rng.uniform(0.0, 1.0, n) ** (1.0 / (1 + j)))   # (some beyond 6)
        tab = np.stack(cols + [np.zeros(n)], axis=1).astype(np.float32)
        signals.append(workloads.Signal(tab, nobs + 1, nexpected=60.0 + 25.0 * j, source_id=j))
    return workloads.Workload(name, nobs, lower, upper, nbins, signals, [], [], np.zeros((0, nobs + 1), np.float32),
                              "Asimov fixture")


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def built(request):
    w = fixture(request.param)
    m = MCMC(w, seed=3, lut_output=False, consume=True, stream=capi.new_stream())
    rows, weights, nexp = ensemble.make_asimov_dataset(w, m.pdfs)
    yield w, m, rows, weights, nexp
    close(m)


def test_rows_look_up_into_the_bins_they_were_made_from(built):
    w, m, rows, weights, nexp = built
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    at = 0
    for j, s in enumerate(w.signals):
        bins, norm = oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, np.zeros(0))
        filled = np.nonzero(np.asarray(bins).reshape(-1))[0]
        assert 0 < filled.size <= int(np.prod(w.nbins)) and norm < s.samples.shape[0]
        mine = rows[at:at + filled.size]
        assert np.all(mine[:, -1] == s.dataset)
        looked_up = np.asarray(oracle.set_eval_points(geom, mine, s.dataset))
        assert np.array_equal(looked_up, filled), j                           # flat index order, each into its own bin
        want = s.nexpected * (norm / float(s.n_mc))
        assert nexp[j] == want
        total = float(np.sum(weights[at:at + filled.size]))
        print(w.name, "signal", j, "rows", filled.size, "weights sum", total, "nexp", want, abs(total - want) / want)
        assert abs(total - want) <= 1e-12 * want
        c = np.asarray(bins).reshape(-1)[filled].astype(np.float64)
        assert np.array_equal(weights[at:at + filled.size], want * c / float(c.sum()))
        at += filled.size
    assert at == rows.shape[0] == weights.size


def group_nll(m, v):
    """The NLL at v through the group's weighted classes and nll_total."""
    m.proposed_vector.set(np.asarray(v, np.float64))
    sums = m.event_partial_sums
    n = m.group.EvalNllAsync(m.stream, m.proposed_vector, m.nexpected, m.n_mc, m.source_id, m.normalizations, sums)
    nll.nll_event_reduce(1, REDUCE_THREADS, m.stream, n, sums, m.event_total_sum)
    nll.nll_total(1, 1, m.stream, m.nparameters, m.proposed_vector, m.nsignals, m.nsources, m.parameter_means,
                  m.parameter_sigma, m.event_total_sum, m.nexpected, m.n_mc, m.source_id, m.normalizations,
                  m.proposed_nll)
    capi.synchronize()
    return float(m.proposed_nll.get()[0])


def test_the_nominal_rates_minimise_the_nll_of_the_asimov_data(built):
    w, m, rows, weights, nexp = built
    m.setup(rows, sync_interval=8, event_weights=weights)
    nominal = w.parameter_means().astype(np.float64)
    at = group_nll(m, nominal)
    assert np.isfinite(at)
    for j in range(w.nsources):
        for f in (0.9, 0.95, 1.05, 1.1):
            v = nominal.copy()
            v[j] *= f
            moved = group_nll(m, v)
            print(w.name, "rate", j, "x", f, "NLL - NLL(nominal)", moved - at, "of", at)
            assert moved > at, (j, f, moved, at)
    assert group_nll(m, nominal) == at


def test_a_fit_of_the_asimov_data_never_goes_below_the_nominal_minimum(built):
    """A whole walk over the weighted rows (ensemble.run_experiment(data=..., event_weights=...)).  The nominal rates
    minimise the NLL (above), so no row of the chain lies below NLL(nominal) -- but for the jump buffer's float32, 6e-8 of
    the NLL.  (How close the best of a few thousand autocorrelated rows comes to the minimum is the sampler's business and
    is printed, not asserted: 0.064 above it was seen at three rates.)"""
    w, m, rows, weights, nexp = built
    m.setup(rows, sync_interval=8, event_weights=weights)
    at = group_nll(m, w.parameter_means().astype(np.float64))
    iv, chain, accepted = ensemble.run_experiment(w, 11, 4000, burnin_fraction=0.2, sync_interval=1000, mcmc=m,
                                                  data=rows, event_weights=weights)
    assert 0 < accepted < 4000 and chain.shape == (4000 - 2 * 800, w.nparameters + 1)   # (both re-tunings drop the steps before them)
    best = float(chain[:, -1].min())
    print(w.name, "best row", chain[np.argmin(chain[:, -1]), :-1], "NLL", best, "NLL(nominal)", at)
    assert best >= at - 1e-6 * abs(at)
    with pytest.raises(ValueError, match="event_weights without the data"):
        ensemble.run_experiment(w, 11, 10, mcmc=m, event_weights=weights)


# ------------------------------------------------------------------ "asimov": true, through both layers' runners
import json
import os
import subprocess

from sxmc_amd import io
from tests.test_io_cpu import EXAMPLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def configured(tmp_path_factory):
    """tests/test_io_cpu.py's EXAMPLE (two histogram signals over one observable and a cut, three floating or fixed
    systematic parameters) with "asimov": true and three experiments configured, its tables on disk; run once through
    tests/cpp/weighted_walk --config (sxmc::ensemble with the key as its option)."""
    work = tmp_path_factory.mktemp("asimov_config")
    rng = np.random.default_rng(0)
    for name, n in (("a.npz", 4000), ("b.npz", 6000)):
        mc = rng.uniform(4, 16, n).astype(np.float32)
        io.write_table(work / name, np.stack([mc + rng.normal(0, 0.5, n).astype(np.float32),
                                              rng.uniform(0, 12, n).astype(np.float32), mc], axis=1),
                       ["energy", "radius", "mc_energy"])
    root = json.loads(io.strip_comments(EXAMPLE))
    root["fit"].update(asimov=True, nexperiments=3, nsteps=600, burnin_fraction=0.2, seed=5)
    (work / "fit.json").write_text(json.dumps(root))
    out = work / "cpp"
    out.mkdir()
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "weighted.mk", "weighted_walk"])
    r = subprocess.run([os.path.join(CPP, "weighted_walk"), "--config", str(work / "fit.json"), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    return work, out, r.stdout


def test_the_cpp_runner_fits_exactly_one_data_set_and_says_so(configured):
    work, out, said = configured
    line = [ln for ln in said.splitlines() if ln.startswith("config\t")][0].split()
    f = dict(zip(line[1::2], line[2::2]))
    assert f["asimov"] == "1" and f["configured"] == "3" and f["ran"] == "1" and f["chains"] == "1"
    assert 0 < int(f["accepted"]) < 600
    assert "Fitting the Asimov data set: %s weighted rows" % f["nevents"] in said
    assert sorted(p for p in os.listdir(out) if p.startswith("chain_")) == ["chain_0.f32"]
    refusal = [ln for ln in said.splitlines() if ln.startswith("refusal: ensemble_lockstep")][0]
    assert "lockstep set has no weighted step end" in refusal


def test_the_cpp_builder_is_the_python_builder_byte_for_byte(configured):
    """sxmc::make_asimov_dataset against ensemble.make_asimov_dataset over the same configuration: rows, weights and
    expected rates as bytes; and on the C++ rows: each looks up into the bin it was made from, the weights of signal j sum
    to nexp_j."""
    work, out, _ = configured
    fc = io.load_config(str(work / "fit.json"))
    w = io.build_workload(fc)
    m = MCMC(w, seed=1, lut_output=False, consume=True)
    try:
        rows, weights, nexp = ensemble.make_asimov_dataset(w, m.pdfs)
    finally:
        close(m)
    got_rows = np.fromfile(out / "asimov_rows.f32", np.float32).reshape(-1, w.nobs + 1)
    got_weights = np.fromfile(out / "asimov_weights.f64", np.float64)
    got_nexp = np.fromfile(out / "asimov_nexp.f64", np.float64)
    assert got_rows.tobytes() == rows.tobytes() and got_weights.tobytes() == weights.tobytes()
    assert got_nexp.tobytes() == np.asarray(nexp, np.float64).tobytes()
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    at = 0
    for j, s in enumerate(w.signals):
        bins, norm = oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, w.parameter_means()[w.nsources:])
        filled = np.nonzero(np.asarray(bins).reshape(-1))[0]
        mine = got_rows[at:at + filled.size]
        assert np.array_equal(np.asarray(oracle.set_eval_points(geom, mine, s.dataset)), filled), j
        want = s.nexpected * (norm / float(s.n_mc))
        assert got_nexp[j] == want and abs(float(np.sum(got_weights[at:at + filled.size])) - want) <= 1e-12 * want
        at += filled.size
    assert at == got_rows.shape[0] == got_weights.size > 0


def test_run_config_and_the_cpp_runner_walk_the_same_chain(configured, tmp_path, monkeypatch):
    """io.run_config with "asimov": true: one experiment although three are configured, said in the report, and the chain
    of tests/cpp/weighted_walk --config byte for byte.  The two layers draw an experiment's seed by different rules and
    their initial widths differ in the last float bit (tests/test_gpu_proposal_cpp.py, cpp_widths, says why): the Python
    walker is handed the C++ run's seed and widths, as that file does, so that what is compared is the runners' handling
    of the key, the two builders and the weighted walk."""
    import io as text_io
    work, out, said = configured
    line = [ln for ln in said.splitlines() if ln.startswith("config\t")][0].split()
    seed = int(dict(zip(line[1::2], line[2::2]))["seed"])
    widths = np.fromfile(out / "widths.f32", np.float32)
    monkeypatch.setattr(MCMC, "initial_jump_widths", lambda self, fixed=None: widths.copy())
    monkeypatch.setattr(MCMC, "reseed", lambda self, _seed: setattr(self, "rngs",
                                                                     nll.make_rngs(self.nparameters, seed, self.stream)))
    report = text_io.StringIO()
    iv, limits, names = io.run_config(str(work / "fit.json"), out_dir=str(tmp_path), report=report)
    assert iv.shape[0] == 1 and len(limits) == 1
    assert "Fitting the Asimov data set: " in report.getvalue()
    assert sorted(p for p in os.listdir(tmp_path) if p.endswith(".npz")) == ["fit_test_0.npz"]
    with np.load(tmp_path / "fit_test_0.npz") as z:
        chain = np.stack([z[n] for n in names], axis=1).astype(np.float32)
    want = np.fromfile(out / "chain_0.f32", np.float32).reshape(-1, len(names))
    assert want.shape[0] == 600 - 2 * 120
    assert chain.tobytes() == want.tobytes(), np.argwhere(chain.view(np.uint32) != want.view(np.uint32))[:4]
    with pytest.raises(ValueError, match="spectra_dir"):
        io.run_config(str(work / "fit.json"), spectra_dir=str(tmp_path / "spectra"))


def test_the_lockstep_runner_refuses_weighted_events():
    with pytest.raises(ValueError, match="lockstep sets have no weighted step end"):
        ensemble.run_experiments_in_lockstep(None, [], 10, [], event_weights=np.ones(3))
