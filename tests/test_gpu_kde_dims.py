"""GPU tests of pdfz::EvalKernel in 1-4 D against the f64 reference (tests/kde_reference.py) with the bound derived
from the kernels' arithmetic: every instantiation of the prepass (NSLOT 1-7), the pair sum (D 1-4, split and unsplit)
and the sampler (D 3 and 4), all four systematic kinds, tile and pitch boundaries, re-set points, point codes, the
domain's edges, extreme bandwidths, domains far from zero or many bandwidths wide, and the normalisation.  Every value
family also shows that its comparison fails against a reference with one planted error."""
import math

import numpy as np
import pytest

from sxmc_amd import pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests.kde_reference import (PLANTS, check_power, check_values, component_cdf, mixture_cdf, moved_in_domain,
                                 ref_kde, truncation_mass)
from tests.test_gpu_kde import gpu_kde
from tests.test_gpu_kde_sample import evaluated, ks_distance, wilson_hilferty_sf

pytestmark = pytest.mark.gpu

CUS = 256   # MI355X: choose_split's resident workgroups are 8 per CU


def choose_split(pitch, ntiles, cus=CUS):
    """kde_plan.h's pair_split: (nsplit, tiles per split)."""
    pblocks, slots = pitch // 256, cus * 8
    best, out = None, (1, ntiles)
    for s in range(1, min(ntiles, max(1, 64 * slots // pblocks)) + 1):
        tps = -(-ntiles // s)
        used = -(-ntiles // tps)
        cost = -(-(pblocks * used) // slots) * tps
        if best is None or cost < best:
            best, out = cost, (used, tps)
    return out


def case(D, extra, n, rng):
    """A table of D observables and `extra` truth fields, each observable its own domain and spread (a mis-strided row
    or swapped observables show), and systematics of all four kinds: a cubic shift, scale, ctscale, and
    resolution_scale reading a truth field that an earlier systematic moved (so the order matters).  The prepass runs
    with NSLOT = D + extra."""
    lower = np.array([-1.0, 0.0, 2.0, -3.0][:D])
    upper = lower + np.array([4.0, 1.5, 6.0, 2.5][:D])
    mid, wid = (lower + upper) / 2, upper - lower
    t = mid + 0.22 * wid * rng.normal(size=(n, D))
    x = t + 0.08 * wid * rng.normal(size=(n, D))
    truth = [t[:, k % D] if k < D else t[:, (D - 1)] for k in range(extra)]
    samples = np.concatenate([x] + [c[:, None] for c in truth], axis=1).astype(np.float32)
    systs = [dict(type="shift", obs=0, pars=[0, 1, 2, 3]), dict(type="scale", obs=D - 1, pars=[4, 5]),
             dict(type="ctscale", obs=1 % D, pars=[6])]
    if extra >= 1:
        systs += [dict(type="shift", obs=D, pars=[7]), dict(type="resolution_scale", obs=0, true_obs=D, pars=[8])]
    elif D >= 2:
        systs.append(dict(type="resolution_scale", obs=0, true_obs=1, pars=[8]))
    if extra >= 2:
        systs.append(dict(type="resolution_scale", obs=1 % D, true_obs=D + 1, pars=[9]))
    if extra >= 3:
        systs.append(dict(type="resolution_scale", obs=D - 1, true_obs=D + 2, pars=[10]))
    params = {0: 0.03, 1: -0.02, 2: 0.004, 3: -0.0005, 4: 0.02, 5: -0.003, 6: 0.05, 7: 0.1, 8: 0.15, 9: -0.1,
              10: 0.08}
    return samples.ravel(), D + extra, lower, upper, systs, params


def points(D, lower, upper, n, rng, other=0.1, outside=0.05):
    p = np.zeros((n, D + 1))
    p[:, :D] = rng.uniform(lower, upper, (n, D))
    p[:, D] = rng.random(n) < other
    out = rng.random(n) < outside
    k = rng.integers(0, D, n)
    p[out, k[out]] = np.where(rng.random(out.sum()) < 0.5, lower[k[out]] - 0.1, upper[k[out]] + 0.1)
    return p.astype(np.float32).ravel()


def hist_norm(samples, nfields, D, lower, upper, systs, params, par_off, par_stride):
    """EvalHist's norm on the same inputs (parameters at the same offset and stride)."""
    hist = pdfz.EvalHist(samples, nfields, D, list(lower), list(upper), [7] * D)
    for s in systs:
        hist.AddSystematic(make_systematic(s))
    pbuf = np.full(par_off + par_stride * (max(params) + 1) + 1, 7.5)
    for q, v in params.items():
        pbuf[par_off + par_stride * q] = v
    norm, par = DeviceArray(np.zeros(1, np.uint32)), DeviceArray(pbuf)
    hist.SetNormalizationBuffer(norm, 0)
    hist.SetParameterBuffer(par, par_off, par_stride)
    hist.EvalAsync(False)
    hist.EvalFinished()
    v = int(norm.get()[0])
    hist.close()
    return v


WORST = {}


def record(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print("worst error / bound so far, %s: %.3g" % (family, WORST[family]))


# ------------------------------------------------------------------ every instantiation
NSLOT_CASES = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (3, 2), (4, 1), (3, 3), (4, 2), (4, 3)]


@pytest.mark.parametrize("D,extra", NSLOT_CASES, ids=["D%d-nslot%d" % (d, d + e) for d, e in NSLOT_CASES])
def test_values_every_nslot(D, extra):
    rng = np.random.default_rng(100 * D + extra)
    samples, nf, lower, upper, systs, params = case(D, extra, 3000, rng)
    pts = points(D, lower, upper, 600, rng)
    scale = [0.9, 1.1, 0.8, 1.2][:D]
    args = (samples, nf, D, lower, upper, scale, systs, params, pts)
    ref = ref_kde(*args)
    got = gpu_kde(*args, par_off=3, par_stride=2, pdf_off=5, pdf_stride=3, norm_off=1)
    assert got["norm"] == ref.norm == hist_norm(samples, nf, D, lower, upper, systs, params, 3, 2)
    assert 2000 < ref.norm < 3000      # (some samples moved out: the domain test and the weights are exercised)
    raw = got["raw"]
    assert np.all(raw[:5] == 12345.0) and np.all(raw[6::3] == 12345.0) and np.all(raw[7::3] == 12345.0)
    record("every NSLOT", check_values(got["values"], ref, "D=%d NSLOT=%d" % (D, D + extra)))
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), [p for p in PLANTS if p != "swap" or D >= 2],
                "D=%d NSLOT=%d" % (D, D + extra))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("nsamples,D", [(2, 3), (255, 4), (256, 3), (257, 4), (4097, 3)])
def test_tile_and_pitch_boundaries(nsamples, D):
    """Sample counts around the 256-row tile, point counts around the 256-point pitch, on one evaluator."""
    rng = np.random.default_rng(nsamples)
    samples, nf, lower, upper, systs, params = case(D, 1, nsamples, rng)
    if nsamples == 2:
        samples = np.concatenate([(lower + upper) / 2 - 0.1, [0.5], (lower + upper) / 2 + 0.2, [0.7]])
        samples = samples.astype(np.float32)
    ev = None
    for npts in (257, 1, 255, 256):
        pts = points(D, lower, upper, npts, rng, other=0.0, outside=0.0)
        args = (samples, nf, D, lower, upper, [1.0] * D, systs, params, pts)
        ref = ref_kde(*args)
        got = gpu_kde(*args, ev=ev)
        ev = got["ev"]
        assert got["norm"] == ref.norm and ev.npoints == npts
        record("tiles", check_values(got["values"], ref, "N=%d E=%d D=%d" % (nsamples, npts, D)))
        if nsamples >= 255 and npts >= 255:
            check_power(got["values"], lambda p: ref_kde(*args, plant=p), label="N=%d E=%d" % (nsamples, npts))


@pytest.mark.parametrize("D", [3, 4])
def test_split_pair_sum(D):
    """A few points against 10^6 samples: the samples split across workgroups."""
    rng = np.random.default_rng(200 + D)
    n = 1000000
    samples, nf, lower, upper, systs, params = case(D, 0, n, rng)
    pts = points(D, lower, upper, 5, rng, other=0.0, outside=0.0)
    assert choose_split(256, -(-n // 256))[0] > 100
    args = (samples, nf, D, lower, upper, [1.0] * D, systs, params, pts)
    ref = ref_kde(*args)
    got = gpu_kde(*args)
    assert got["norm"] == ref.norm
    record("split", check_values(got["values"], ref, "split D=%d" % D))
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), ("bandwidth", "untruncated", "swap"), "split")


@pytest.mark.parametrize("D", [3, 4])
def test_unsplit_pair_sum(D):
    """2048 point blocks over two tiles: choose_split keeps the tiles in one workgroup; every 64th point compared."""
    rng = np.random.default_rng(300 + D)
    samples, nf, lower, upper, systs, params = case(D, 1, 400, rng)
    npts = 2048 * 256 - 100
    assert choose_split(2048 * 256, 2) == (1, 2)
    pts = points(D, lower, upper, npts, rng, other=0.0, outside=0.0)
    got = gpu_kde(samples, nf, D, lower, upper, [1.0] * D, systs, params, pts)
    sub = pts.reshape(npts, D + 1)[::64]
    args = (samples, nf, D, lower, upper, [1.0] * D, systs, params, sub.ravel())
    ref = ref_kde(*args)
    assert got["norm"] == ref.norm
    record("unsplit", check_values(got["values"][::64], ref, "unsplit D=%d" % D))
    check_power(got["values"][::64], lambda p: ref_kde(*args, plant=p), label="unsplit")


def test_reset_points_on_one_evaluator():
    """Many points, few (more splits), none, then more than at first (the buffers grow): values right after each
    (of many points, every stride-th compared)."""
    rng = np.random.default_rng(400)
    D = 3
    samples, nf, lower, upper, systs, params = case(D, 2, 4000, rng)
    assert choose_split(40192, 16)[0] < choose_split(256, 16)[0]
    ev = None
    for npts, stride in ((40000, 8), (7, 1), (0, 1), (60000, 12)):
        pts = points(D, lower, upper, npts, rng)
        got = gpu_kde(samples, nf, D, lower, upper, [1.0] * D, systs, params, pts, ev=ev)
        ev = got["ev"]
        sub = pts.reshape(npts, D + 1)[::stride].ravel()
        ref = ref_kde(samples, nf, D, lower, upper, [1.0] * D, systs, params, sub)
        assert got["norm"] == ref.norm and ev.npoints == npts
        if npts == 0:
            assert np.all(got["raw"] == 12345.0)
            continue
        record("re-set points", check_values(got["values"][::stride], ref, "re-set E=%d" % npts))


# ------------------------------------------------------------------ point codes
@pytest.mark.parametrize("D", [3, 4])
def test_point_codes(D):
    rng = np.random.default_rng(500 + D)
    samples, nf, lower, upper, systs, params = case(D, 1, 2000, rng)
    mid = ((lower + upper) / 2).astype(np.float32)
    rows = [np.append(mid, 0), np.append(mid, 1)]           # own data set, another one
    for k in range(D):
        for bad in (lower[k] - 0.01, upper[k], np.nan, np.inf):
            p = np.append(mid, 0).astype(np.float32)
            p[k] = bad
            rows.append(p)
            q = p.copy()
            q[D] = 1
            rows.append(q)                                   # outside: NaN whatever the data set
    pts = np.array(rows, np.float32).ravel()
    args = (samples, nf, D, lower, upper, [1.0] * D, systs, params, pts)
    got = gpu_kde(*args, dataset=0)
    v = got["values"]
    assert v[0] > 0 and v[1] == 0.0 and np.all(np.isnan(v[2:]))
    check_values(v, ref_kde(*args), "codes D=%d" % D)
    # every sample moved out of the domain: norm 0, NaN for the data set's points, 0 for another data set's
    gone = dict(params)
    gone[0] = 100.0
    got = gpu_kde(samples, nf, D, lower, upper, [1.0] * D, systs, gone, pts, ev=got["ev"])
    v = got["values"]
    assert got["norm"] == 0 and math.isnan(v[0]) and v[1] == 0.0 and np.all(np.isnan(v[2:]))


# ------------------------------------------------------------------ edges
def test_samples_on_the_edges_and_moved_across_them():
    rng = np.random.default_rng(600)
    D = 3
    lower, upper = np.array([0.0, -1.0, 10.0]), np.array([1.0, 1.0, 10.5])
    top = np.nextafter(upper.astype(np.float32), np.float32(-np.inf))
    x = np.minimum(rng.uniform(lower, upper, (3000, D)).astype(np.float32), top)
    for d in range(D):
        x[d * 300:d * 300 + 100, d] = np.float32(lower[d])
        x[d * 300 + 100:d * 300 + 200, d] = top[d]
    assert np.all(top.astype(np.float64) < upper)
    pts = points(D, lower, upper, 800, rng, outside=0.0)
    edge = np.zeros((64, D + 1), np.float32)
    edge[:, :D] = rng.uniform(lower, upper, (64, D))
    edge[:32, 0], edge[32:, 1] = np.float32(lower[0]), top[1]
    pts = np.concatenate([pts, edge.ravel()])
    args = (x.ravel(), D, D, lower, upper, [0.7] * D, [], {}, pts)
    ref = ref_kde(*args)
    got = gpu_kde(*args)
    assert got["norm"] == ref.norm == 3000
    record("edges", check_values(got["values"], ref, "samples on the edges"))
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), label="edges")
    # a shift moves a sample across an edge: its weight is the moved sample's, and those moved out drop
    systs = [dict(type="shift", obs=0, pars=[0]), dict(type="shift", obs=2, pars=[1])]
    for params in ({0: 0.02, 1: -0.01}, {0: -0.013, 1: 0.004}):
        args = (x.ravel(), D, D, lower, upper, [0.7] * D, systs, params, pts)
        ref = ref_kde(*args)
        got = gpu_kde(*args, ev=got["ev"] if params[0] < 0 else None)
        assert got["norm"] == ref.norm < 3000
        record("edges", check_values(got["values"], ref, "moved across an edge %s" % params))


@pytest.mark.parametrize("scale", [0.01, 1e3])
def test_extreme_bandwidths(scale):
    """0.01: most pairs underflow (the absolute floor); 10^3: a nearly flat pdf with large weights."""
    rng = np.random.default_rng(700)
    D = 2
    samples, nf, lower, upper, systs, params = case(D, 1, 5000, rng)
    pts = points(D, lower, upper, 2000, rng)
    # and points on the moved samples nearest each edge, where the truncation weights show at any bandwidth
    s = moved_in_domain(samples, nf, D, lower, upper, systs, params)
    near = np.concatenate([s[np.argmin(s[:, d])][None] for d in range(D)] + [s[np.argmax(s[:, d])][None] for d in range(D)])
    near = np.concatenate([near, np.zeros((len(near), 1))], axis=1).astype(np.float32)
    pts = np.concatenate([pts, near.ravel()])
    args = (samples, nf, D, lower, upper, [scale] * D, systs, params, pts)
    ref = ref_kde(*args)
    got = gpu_kde(*args)
    assert got["norm"] == ref.norm
    v = ref.values[~np.isnan(ref.values) & (ref.values > 0)]
    print("scale %g: h %s, c_max %.3g, values %.3g .. %.3g" % (scale, ref.h, ref.c_max, v.min(), v.max()))
    record("bandwidth x%g" % scale, check_values(got["values"], ref, "bandwidth x%g" % scale))
    # (at 10^3 the truncated kernels are flat over the domain, w / h independent of h: a wrong h changes nothing)
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), [p for p in PLANTS if scale < 1 or p != "bandwidth"],
                "bandwidth x%g" % scale)


def test_domain_far_from_zero():
    """lower = 10^4, width 10 (energies in keV from 10 MeV, say): the coordinates are measured from lower."""
    rng = np.random.default_rng(800)
    x = np.stack([rng.normal(1e4 + 5, 2.0, 4000), rng.normal(0.0, 1.0, 4000)], axis=1).astype(np.float32)
    lower, upper = [1e4, -3.0], [1e4 + 10, 3.0]
    pts = np.stack([rng.uniform(1e4, 1e4 + 10, 2000), rng.uniform(-3, 3, 2000), np.zeros(2000)], axis=1)
    args = (x.ravel(), 2, 2, lower, upper, [1.0, 1.0], [dict(type="scale", obs=0, pars=[0])], {0: 1e-4},
            pts.astype(np.float32).ravel())
    ref = ref_kde(*args)
    got = gpu_kde(*args)
    assert got["norm"] == ref.norm
    record("far from zero", check_values(got["values"], ref, "lower 1e4"))
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), label="far from zero")


@pytest.mark.parametrize("centre", [100.0, 1000.0])
def test_data_many_bandwidths_from_lower(centre):
    """The data lie `centre` bandwidths from lower (a radius in mm from 0, say): the f32 coordinates' error grows with
    (x - lower) / h, and the bound with it."""
    rng = np.random.default_rng(900)
    n = 4000
    s = rng.normal(0.0, 1.0, (n, 2))
    h = 1.0 * n ** (-1.0 / 6)
    x = np.stack([centre * h + s[:, 0], s[:, 1]], axis=1).astype(np.float32)
    lower, upper = [0.0, -4.0], [centre * h + 5.0, 4.0]
    pts = np.stack([rng.uniform(centre * h - 3, centre * h + 3, 2000), rng.uniform(-3, 3, 2000), np.zeros(2000)],
                   axis=1)
    args = (x.ravel(), 2, 2, lower, upper, [1.0, 1.0], [], {}, pts.astype(np.float32).ravel())
    ref = ref_kde(*args)
    got = gpu_kde(*args)
    assert got["norm"] == ref.norm and ref.c_max > 0.8 * centre
    record("%g bandwidths from lower" % centre, check_values(got["values"], ref, "%g h from lower" % centre))
    check_power(got["values"], lambda p: ref_kde(*args, plant=p), label="%g h from lower" % centre)


# ------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("D,m", [(3, 48), (4, 22)])
def test_normalisation_3d_4d(D, m):
    """The midpoint rule over the domain integrates to 1 within its error bound: per observable at most
    step^2 / 24 * w int |phi''| / h^2 = 0.968 w step^2 / (24 h^2) for a component of weight w."""
    rng = np.random.default_rng(1000 + D)
    lower, upper = np.zeros(D), np.array([1.0, 2.0, 1.5, 1.0][:D])
    x = rng.beta(0.8, 0.8, (400, D)) * upper
    x = x.astype(np.float32)
    c = [(np.arange(m) + 0.5) / m * upper[d] for d in range(D)]
    grid = np.stack(np.meshgrid(*c, indexing="ij"), axis=-1).reshape(-1, D)
    pts = np.concatenate([grid, np.zeros((len(grid), 1))], axis=1).astype(np.float32).ravel()
    got = gpu_kde(x.ravel(), D, D, lower, upper, [2.0] * D, [], {}, pts)
    h = got["ev"].Bandwidths()
    step = upper / m
    integral = float(np.sum(got["values"].astype(np.float64)) * np.prod(step))
    w = 1.0 / truncation_mass(x, h, lower, upper)
    tol = 0.968 * float(np.mean(w)) * float(np.sum(step ** 2 / (24 * h ** 2))) + 1e-5
    print("%d-D integral %.8f (tolerance %.3g, h %s)" % (D, integral, tol, h))
    assert abs(integral - 1.0) <= tol
    assert tol < 0.02


# ------------------------------------------------------------------ draws in 3-D and 4-D
def test_law_3d_with_systematics():
    """Chi-square over a 3-D grid of separable truncated CDFs, NSLOT 5; the check sees a clamped Gaussian."""
    rng = np.random.default_rng(1100)
    D = 3
    samples, nf, lower, upper, systs, params = case(D, 2, 3000, rng)
    got = evaluated(samples, nf, D, lower, upper, [1.0] * D, systs, params)
    ev = got["ev"]
    s = moved_in_domain(samples, nf, D, lower, upper, systs, params)
    assert ev.SamplePool() == got["norm"] == len(s)
    h = ev.Bandwidths()
    N = 400000
    events = ev.RandomSample(N, 31337)
    x = events[:, :D].astype(np.float64)
    assert np.all((x >= lower) & (x < upper)) and np.all(events[:, D] == 0.0)
    edges = [np.linspace(lower[d], upper[d], 9) for d in range(D)]
    A = [np.diff(component_cdf(edges[d], s[:, d], h[d], lower[d], upper[d]), axis=0) for d in range(D)]   # [8, n]
    expect = N * np.einsum("in,jn,kn->ijk", A[0], A[1], A[2]) / len(s)
    assert abs(expect.sum() - N) < 1e-6 * N
    use = expect >= 5

    def pvalue(xs):
        counts, _ = np.histogramdd(xs, bins=edges)
        chi2 = float((((counts - expect) ** 2) / expect)[use].sum())
        return wilson_hilferty_sf(chi2, int(use.sum()) - 1), counts

    p, counts = pvalue(x)
    print("3-D chi2 p = %.3g over %d cells" % (p, int(use.sum())))
    assert p > 1e-4
    assert counts[~use].sum() <= 5 * max(1.0, expect[~use].sum()) + 20
    r2 = np.random.default_rng(5)
    wrong = s[r2.integers(0, len(s), N)] + h * r2.normal(size=(N, D))
    wrong = np.clip(wrong, lower, np.nextafter(upper, lower))
    assert pvalue(wrong)[0] < 1e-4
    # cuts: every event inside them; the same seed, the same bits
    lo = (lower + 0.3 * (upper - lower)).astype(np.float32)
    hi = (lower + 0.6 * (upper - lower)).astype(np.float32)
    c = ev.RandomSample(50000, 8, lowers=lo, uppers=hi)[:, :D]
    assert np.all((c >= lo) & (c <= hi))
    a, b = ev.RandomSample(50000, 9), ev.RandomSample(50000, 9)
    assert a.tobytes() == b.tobytes()


def test_law_4d_marginals():
    """KS of each marginal against its exact mixture CDF (the components are separable, so the marginal is the 1-D
    mixture of the moved in-domain samples' truncated Gaussians)."""
    rng = np.random.default_rng(1200)
    D = 4
    samples, nf, lower, upper, systs, params = case(D, 3, 2000, rng)
    got = evaluated(samples, nf, D, lower, upper, [1.2, 0.9, 1.0, 1.5], systs, params)
    ev = got["ev"]
    s = moved_in_domain(samples, nf, D, lower, upper, systs, params)
    assert ev.SamplePool() == len(s)
    h = ev.Bandwidths()
    N = 100000
    x = ev.RandomSample(N, 2024)[:, :D].astype(np.float64)
    assert np.all((x >= lower) & (x < upper))
    for d in range(D):
        ks = ks_distance(x[:, d], s[:, d], h[d], lower[d], upper[d]) * math.sqrt(N)
        print("4-D marginal %d: KS D sqrt(N) = %.3f" % (d, ks))
        assert ks < 1.95
    # power: the marginal of another observable, or an untruncated clamp, fails
    grid = np.linspace(lower[0], upper[0], 4001)
    assert np.max(np.abs(mixture_cdf(grid, s[:, 0], h[0] * 1.3, lower[0], upper[0])
                         - mixture_cdf(grid, s[:, 0], h[0], lower[0], upper[0]))) * math.sqrt(N) > 1.95


def test_print_worst_ratios():
    """(Last in the file: the worst error / bound of every value family above.)"""
    for k, v in sorted(WORST.items()):
        print("worst error / bound, %s: %.3g" % (k, v))
        assert v <= 1.0
