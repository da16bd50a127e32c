"""GPU tests of the two device projections (include/sxmc_hip.h: sxmc_hist_project, sxmc_kde_project) through
pdfz.EvalHist.ProjectCounts / Project and pdfz.EvalKernel.Project.

* Histogram: the marginal along every observable equals, exactly, the bins GetBins() returns summed over the other
  axes on the host, and the CPU oracle's bins summed the same way -- 1 to 4 observables, an axis of one bin, total bin
  counts that are no multiple of the workgroup, axes past the LDS path (200 000 bins; 70 000 x 2), 70 000 samples in one
  bin (more than 16 bits).  State: refused while the bins are not valid, the same twice, GetBins() unchanged.
* Kernel density: against tests/project_reference.py, per bin |d| <= 1e-11 from the f32 rows the prepass leaves (at most
  4096 f64 terms of at most 1/N each: N 2^-53 times a few operations is about 4e-12; libm and the device's erfc differ
  by a few ulp) and |d| <= 0.4 u_max 2^-24 / mass_min from the unrounded samples (what rounding the rows to f32 can
  move: a row's u moves by at most u 2^-24, a share by at most the kernel's peak density 0.399 / mass times that); the
  sum is 1 within 1e-12; a reference with the bandwidth times 1.01 fails the first comparison."""
import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests.kde_reference import ref_kde
from tests.project_reference import U24, ref_kde_marginal, ref_kde_marginal_exact
from tests.test_gpu_kde_dims import case

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ histogram
def hist_table(rng, D, n):
    """D observables in [0, 1) (a few per cent outside) and one truth field."""
    t = rng.uniform(-0.02, 1.02, (n, D))
    x = t + 0.03 * rng.normal(size=(n, D))
    return np.concatenate([x, t[:, :1]], axis=1).astype(np.float32)


HIST_SYSTS = [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=0, pars=[1]),
              dict(type="resolution_scale", obs=0, true_obs=-1, pars=[2])]
HIST_PARAMS = [0.013, -0.021, 0.08]


def filled(table, D, nbins, systs, params, lower=None, upper=None):
    """(evaluator after EvalAsync(False), its buffers, the oracle's bins) for a table of D observables + fields."""
    nf = table.shape[1]
    lower = [0.0] * D if lower is None else lower
    upper = [1.0] * D if upper is None else upper
    systs = [dict(s, true_obs=D) if s.get("true_obs") == -1 else s for s in systs]
    ev = pdfz.EvalHist(table.ravel(), nf, D, lower, upper, nbins)
    for s in systs:
        ev.AddSystematic(make_systematic(s))
    norm, par = DeviceArray.zeros(1, np.uint32), DeviceArray(np.asarray(params + [0.0], np.float64))
    ev.SetNormalizationBuffer(norm)
    ev.SetParameterBuffer(par)
    ev.EvalAsync(False)
    ev.EvalFinished()
    want, _ = oracle.bin_samples(oracle.HistGeometry(lower, upper, nbins), table.ravel(), nf, systs,
                                 np.asarray(params + [0.0]))
    return ev, (norm, par), want


def check_hist(ev, nbins, want):
    cube = ev.GetBins().reshape(nbins).astype(np.uint64)
    assert np.array_equal(cube.ravel(), want.astype(np.uint64))
    D = len(nbins)
    total = int(cube.sum())
    for obs in range(D):
        marg = cube.sum(axis=tuple(a for a in range(D) if a != obs), dtype=np.uint64)
        got = ev.ProjectCounts(obs)
        assert got.dtype == np.uint64 and got.shape == (nbins[obs],)
        assert np.array_equal(got, marg), "observable %d of %s" % (obs, nbins)
        assert np.array_equal(ev.ProjectCounts(obs), got)                     # the same twice
        share = ev.Project(obs, nbins[obs])
        assert np.array_equal(share, marg / float(total)) and abs(share.sum() - 1.0) <= 1e-12
    assert np.array_equal(ev.GetBins().reshape(nbins).astype(np.uint64), cube)   # the histogram is untouched
    return total


@pytest.mark.parametrize("nbins", [[7], [5, 3], [4, 3, 5], [3, 2, 4, 2], [1, 9]], ids=lambda b: "x".join(map(str, b)))
def test_hist_marginals_small(nbins):
    D = len(nbins)
    table = hist_table(np.random.default_rng(10 + D + nbins[0]), D, 1000)
    ev, keep, want = filled(table, D, nbins, HIST_SYSTS, HIST_PARAMS)
    total = check_hist(ev, nbins, want)
    assert 700 < total < 1000            # (some samples moved out: the marginals are of a real evaluation)
    ev.close()


@pytest.mark.parametrize("nbins", [[200000], [70000, 2]], ids=lambda b: "x".join(map(str, b)))
def test_hist_marginals_past_the_lds_path(nbins):
    D = len(nbins)
    table = hist_table(np.random.default_rng(20 + D), D, 30000)
    ev, keep, want = filled(table, D, nbins, HIST_SYSTS, HIST_PARAMS)
    check_hist(ev, nbins, want)
    ev.close()


def test_hist_one_bin_beyond_sixteen_bits():
    n = 70000
    table = np.tile(np.array([[0.41, 0.77, 0.41]], np.float32), (n, 1))
    ev, keep, want = filled(table, 2, [3, 4], [], [])
    assert want.max() == n > 65535
    check_hist(ev, [3, 4], want)
    assert np.array_equal(ev.ProjectCounts(0), [0, n, 0]) and np.array_equal(ev.ProjectCounts(1), [0, 0, 0, n])
    ev.close()


def test_hist_refused_while_the_bins_are_not_valid_and_bad_arguments():
    rng = np.random.default_rng(31)
    nbins = [300, 250]                                       # 75 000 bins: a look-up counts only the event bins
    table = hist_table(rng, 2, 5000)
    ev, keep, want = filled(table, 2, nbins, HIST_SYSTS, HIST_PARAMS)
    assert int(ev.ProjectCounts(1).sum()) == int(want.sum())
    pts = np.concatenate([rng.uniform(0, 1, (200, 2)), np.zeros((200, 1))], axis=1).astype(np.float32)
    out = DeviceArray.zeros(200, np.float32)
    ev.SetEvalPoints(pts)
    ev.SetPDFValueBuffer(out)
    ev.EvalAsync(True)
    ev.EvalFinished()
    with pytest.raises(capi.SxmcError) as err:
        ev.ProjectCounts(0)
    assert err.value.code == capi.ERR_STATE and "the histogram is not filled" in str(err.value)
    with pytest.raises(capi.SxmcError) as err:
        ev.GetBins()
    assert err.value.code == capi.ERR_STATE
    ev.EvalAsync(False)                                      # recovery
    ev.EvalFinished()
    check_hist(ev, nbins, want)
    # bad arguments, straight at the entry point
    lib, buf = capi.load(), np.zeros(300, np.uint64)
    assert lib.sxmc_hist_project(ev.handle, 0, None, 300) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(ev.handle, -1, capi.ptr(buf), 300) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(ev.handle, 2, capi.ptr(buf), 300) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(ev.handle, 0, capi.ptr(buf), 250) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(ev.handle, 1, capi.ptr(buf), 300) == capi.ERR_INVALID
    with pytest.raises(pdfz.Error):
        ev.Project(0, 299)
    ev.close()


# ------------------------------------------------------------------ kernel density
NBINS = (1, 63, 64, 65, 257)


def kde_evaluated(samples, nf, D, lower, upper, scale, systs, params):
    ev = pdfz.EvalKernel(samples, nf, D, list(lower), list(upper), scale)
    for s in systs:
        ev.AddSystematic(make_systematic(s))
    pbuf = np.zeros(max(params.keys(), default=0) + 2)
    for q, v in params.items():
        pbuf[q] = v
    norm, par = DeviceArray.zeros(1, np.uint32), DeviceArray(pbuf)
    ev.SetNormalizationBuffer(norm)
    ev.SetParameterBuffer(par)
    return ev, norm, par, pbuf


def check_kde(ev, args, D, nbins_list=NBINS, label=""):
    """Every observable and bin count against both references; returns the worst |d| against the rounded rows."""
    worst = 0.0
    for obs in range(D):
        for nb in nbins_list:
            got = ev.Project(obs, nb)
            assert got.dtype == np.float64 and got.shape == (nb,)
            want = ref_kde_marginal(*args, obs, nb)
            exact, u_max, mass_min = ref_kde_marginal_exact(*args, obs, nb)
            d = float(np.abs(got - want).max())
            dx = float(np.abs(got - exact).max())
            tol_exact = 0.4 * u_max * U24 / mass_min
            print("%s obs %d nbins %d: |d| %.3g (rows) %.3g (exact, tolerance %.3g), sum - 1 %.3g"
                  % (label, obs, nb, d, dx, tol_exact, got.sum() - 1.0))
            assert d <= 1e-11
            assert dx <= tol_exact
            assert abs(got.sum() - 1.0) <= 1e-12
            assert ev.Project(obs, nb).tobytes() == got.tobytes()              # two calls, the same bits
            if nb > 1:                                                          # power: a bandwidth 1 % off shows
                off = ref_kde_marginal(*args, obs, nb, bandwidth_factor=1.01)
                assert float(np.abs(got - off).max()) > 1e-11
            worst = max(worst, d)
    return worst


@pytest.mark.parametrize("N", [2, 255, 256, 257, 1000])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_kde_marginals(D, N):
    """All four systematic kinds (tests/test_gpu_kde_dims.case: cubic shift, scale, cos-theta scale, resolution scale on
    a truth field another systematic moved), sample counts around the 256-row tile."""
    rng = np.random.default_rng(1000 * D + N)
    samples, nf, lower, upper, systs, params = case(D, 1, max(N, 8), rng)
    if N == 2:
        mid = (lower + upper) / 2
        samples = np.concatenate([mid - 0.1, [0.5], mid + 0.2, [0.7]]).astype(np.float32)
    scale = [0.9, 1.1, 0.8, 1.2][:D]
    ev, norm, par, pbuf = kde_evaluated(samples, nf, D, lower, upper, scale, systs, params)
    with pytest.raises(capi.SxmcError) as err:                                 # nothing evaluated yet
        ev.Project(0, 4)
    assert err.value.code == capi.ERR_STATE
    ev.EvalAsync(False)
    ev.EvalFinished()
    args = (samples, nf, D, lower, upper, scale, systs, pbuf)
    check_kde(ev, args, D, label="D=%d N=%d" % (D, N))
    ev.close()


def test_kde_a_third_moved_out_and_a_sample_at_lower():
    rng = np.random.default_rng(77)
    D, n = 2, 900
    lower, upper = np.array([0.0, -1.0]), np.array([4.0, 1.0])
    x = np.stack([rng.uniform(0.05, 3.95, n), rng.uniform(-0.9, 0.9, n)], axis=1).astype(np.float32)
    x[5] = [0.0, -1.0]                                                          # exactly at lower, in both observables
    systs = [dict(type="shift", obs=0, pars=[0])]
    ev, norm, par, pbuf = kde_evaluated(x.ravel(), 2, D, lower, upper, [1.0, 1.0], systs, {0: 0.0})
    args = (x.ravel(), 2, D, lower, upper, [1.0, 1.0], systs, pbuf)
    ev.EvalAsync(False)
    ev.EvalFinished()
    assert int(norm.get()[0]) == n == ev.SamplePool()                           # (the sample at lower is inside)
    check_kde(ev, args, D, (1, 10, 100), "at lower")
    # a shift that pushes about a third of the samples past upper
    pbuf[0] = 1.3
    par.set(pbuf)
    ev.EvalAsync(False)
    ev.EvalFinished()
    left = int(norm.get()[0])
    assert 0.6 * n < left < 0.72 * n
    check_kde(ev, args, D, (1, 10, 100), "a third out")
    # ... and one that leaves nothing: zeros
    pbuf[0] = 100.0
    par.set(pbuf)
    ev.EvalAsync(False)
    ev.EvalFinished()
    assert int(norm.get()[0]) == 0
    for obs in range(D):
        assert np.array_equal(ev.Project(obs, 17), np.zeros(17))
    # bad arguments
    lib, buf = capi.load(), np.zeros(8)
    assert lib.sxmc_kde_project(ev.handle, 0, 8, None) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(ev.handle, -1, 8, capi.ptr(buf)) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(ev.handle, 2, 8, capi.ptr(buf)) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(ev.handle, 0, 0, capi.ptr(buf)) == capi.ERR_INVALID
    with pytest.raises(pdfz.Error):
        ev.Project(0, 0)
    ev.close()


def test_kde_marginal_is_the_integral_of_the_evaluated_pdf():
    """D = 2, N = 300, 8 bins: the pdf values EvalAsync(True) returns on a 32 x 32 grid per bin (32 across the bin, 32
    across the whole of the other observable), integrated by the midpoint rule, against Project.  With Q the
    quadrature, M the analytic marginal and P the projection, |Q_gpu - P| <= |Q_gpu - Q_ref| + |Q_ref - M| + |M - P|:
    the evaluator's documented value bound (tests/kde_reference.py) integrated over the grid, the reference's own
    quadrature error on that grid, and the projection's tolerance."""
    rng = np.random.default_rng(5)
    D, N, nb, m = 2, 300, 8, 32
    samples, nf, lower, upper, systs, params = case(D, 1, N, rng)
    scale = [1.0, 1.0]
    ev, norm, par, pbuf = kde_evaluated(samples, nf, D, lower, upper, scale, systs, params)
    args = (samples, nf, D, lower, upper, scale, systs, pbuf)
    for obs in range(D):
        other = 1 - obs
        w_bin, w_other = (upper[obs] - lower[obs]) / nb, upper[other] - lower[other]
        a = lower[obs] + (np.arange(nb * m) + 0.5) * (w_bin / m)
        b = lower[other] + (np.arange(m) + 0.5) * (w_other / m)
        grid = np.zeros((nb * m, m, D + 1))
        grid[:, :, obs] = a[:, None]
        grid[:, :, other] = b[None, :]
        pts = grid.reshape(-1, D + 1).astype(np.float32)
        out = DeviceArray.zeros(len(pts), np.float32)
        ev.SetEvalPoints(pts)
        ev.SetPDFValueBuffer(out)
        ev.EvalAsync(True)
        ev.EvalFinished()
        ref = ref_kde(*args[:7], params, pts.ravel())
        area = w_bin * w_other
        q_gpu = out.get().astype(np.float64).reshape(nb, m * m).mean(axis=1) * area
        q_ref = ref.values.reshape(nb, m * m).mean(axis=1) * area
        value_bound = ref.bound.reshape(nb, m * m).mean(axis=1) * area
        exact, u_max, mass_min = ref_kde_marginal_exact(*args, obs, nb)
        got = ev.Project(obs, nb)
        tol = value_bound + np.abs(q_ref - exact) + 0.4 * u_max * U24 / mass_min
        err = np.abs(q_gpu - got)
        print("obs %d: |quadrature - Project| %s, tolerance %s" % (obs, err.max(), tol.min()))
        assert np.all(err <= tol)
        assert np.abs(q_ref - exact).max() < 1e-3           # (the grid resolves the kernels: the check has teeth)
    ev.close()
