"""Weighted Monte Carlo samples in pdfz::EvalKernel on the device (sxmc_kde_create_weighted, the laws in
include/sxmc_hip.h) against tests/kde_weighted_reference.py: all m = 8 gives the unweighted evaluator's bytes, small
multiplicities give the repeated table's values, the adaptive factors, the cutoff's statistics and envelope, the
projection, a shared evaluator, and the planted references, each of which the device's output must fail."""
import numpy as np
import pytest

from sxmc_amd import capi, pdfz
from sxmc_amd.mcmc import make_systematic
from tests import kde_weighted_reference as W
from tests.kde_cutoff_reference import replay_visits
from tests.kde_reference import TILE, compare, ref_transform
from tests.test_gpu_kde import gpu_kde

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 11


def evaluator(c, m=None, alpha=0.0, scale=None):
    ev = pdfz.EvalKernel(c.table.ravel(), c.nfields, c.D, c.lower, c.upper, c.scale if scale is None else scale,
                         dataset=c.dataset, bandwidth_sensitivity=alpha, multiplicities=m)
    for s in c.systs:
        ev.AddSystematic(make_systematic(s))
    return ev


def run(ev, c, points=None, **kw):
    pts = c.points if points is None else points
    return gpu_kde(None, None, c.D, c.lower, c.upper, None, None, W.PARAMS, pts.ravel(), ev=ev, **kw)


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------ 1. all m = 8: the unweighted evaluator's bytes
# (every shape, fixed and adaptive: tests/test_kde_weighted_reference_cpu.py asserts their q' < 100, the factors in)
BYTE_CASES = [(D, N, E, alpha) for D, N, E in W.SHAPES for alpha in (0.0, 0.5)]


@pytest.mark.parametrize("D,N,E,alpha", BYTE_CASES)
def test_all_eights_give_the_unweighted_bytes(D, N, E, alpha):
    c = W.case(D, N, E)
    plain, eight = evaluator(c, None, alpha), evaluator(c, np.full(N, 8, np.uint32), alpha)
    assert not plain.HasSampleMultiplicities() and eight.HasSampleMultiplicities()
    assert plain.SampleTotal() == N and eight.SampleTotal() == 8 * N
    assert np.all(plain.SampleMultiplicities() == 1) and np.all(eight.SampleMultiplicities() == 8)
    assert eight.EffectiveSamples() == plain.EffectiveSamples()
    assert same_bytes(plain.Bandwidths(), eight.Bandwidths())
    assert same_bytes(plain.LocalFactors(), eight.LocalFactors())
    assert np.all(plain.LocalFactors() == 1.0) == (alpha == 0.0)
    a, b = run(plain, c), run(eight, c)
    assert 0 < a["norm"] < N and b["norm"] == 8 * a["norm"]
    assert same_bytes(a["values"], b["values"])
    assert plain.SamplePool() == eight.SamplePool() == a["norm"]
    for obs in range(D):
        assert same_bytes(plain.Project(obs, 7), eight.Project(obs, 7))
    assert same_bytes(plain.RandomSample(500, SEED), eight.RandomSample(500, SEED))
    lo, hi = np.full(D, -1.0, np.float32), np.full(D, 1.2, np.float32)
    assert same_bytes(plain.RandomSample(300, 7, lo, hi), eight.RandomSample(300, 7, lo, hi))    # (cuts force redraws)
    for ev in (plain, eight):
        ev.SetCutoff(4.0)
    a, b = run(plain, c), run(eight, c)
    assert same_bytes(a["values"], b["values"]) and b["norm"] == 8 * a["norm"]
    assert plain.CutoffStats() == eight.CutoffStats() and plain.CutoffStats()[0] > 0
    ta, tb = plain.CutoffBoxes(), eight.CutoffBoxes()
    assert same_bytes(ta[0], tb[0]) and same_bytes(ta[1], tb[1])
    plain.close()
    eight.close()


# ------------------------------------------------------------------ 2. m in {0..3}: the reference, the repeated table
@pytest.mark.parametrize("D,N,E", W.SHAPES)
def test_small_multiplicities(D, N, E):
    c = W.case(D, N, E)
    m = W.small_multiplicities(c)
    ev = evaluator(c, m)
    got = run(ev, c)
    h = ev.Bandwidths()
    ref = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                             dataset=c.dataset)
    assert np.max(np.abs(h - ref.h) / ref.h) <= 1e-13
    assert got["norm"] == ref.norm and ev.SampleTotal() == int(m.sum())
    assert ev.EffectiveSamples() == W.law_bandwidths(c.table, c.nfields, D, c.lower, c.upper, c.scale, m)["n_eff"]
    ok, ratio, rel = compare(got["values"], ref)
    print("D=%d N=%d E=%d: %.3g x the bound, relative %.3g" % (D, N, E, ratio, rel))
    assert ok
    # the evaluator over the table in which row i stands m_i times, at the same bandwidths
    rep = W.repeated_table(c.table, c.nfields, m)
    cr = W.Case(D, c.nfields, rep, c.lower, c.upper, c.scale, c.systs, c.points, c.dataset)
    probe = evaluator(cr)
    evr = evaluator(cr, scale=c.scale * (h / probe.Bandwidths()))
    probe.close()
    hr = evr.Bandwidths()
    assert np.max(np.abs(hr - h) / h) <= 8 * 2.0 ** -52
    gotr = run(evr, cr)
    refr = W.ref_kde_weighted(rep, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points,
                              np.ones(len(rep), np.uint32), dataset=c.dataset, h=hr)
    assert gotr["norm"] == got["norm"]
    v, vr = got["values"].astype(np.float64), gotr["values"].astype(np.float64)
    assert np.array_equal(np.isnan(v), np.isnan(vr))
    live = ~np.isnan(v)
    excess = np.abs(v[live] - vr[live]) - (ref.bound[live] + refr.bound[live] + 1e-12 * np.abs(v[live]))
    assert np.all(excess <= 0), float(excess.max())
    # 7. the planted references: the device's values fail each
    for plant in W.PLANTS:
        bad = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                                 dataset=c.dataset, plant=plant)
        okp, ratio, _ = compare(got["values"], bad)
        print("  plant %s: %.3g x the bound" % (plant, ratio))
        assert not okp, plant
    ev.close()
    evr.close()


# ------------------------------------------------------------------ 3. adaptive
@pytest.mark.parametrize("D,N,E", W.SHAPES[:5])
def test_adaptive_small_multiplicities(D, N, E):
    c = W.case(D, N, E)
    m = W.small_multiplicities(c)
    ev = evaluator(c, m, 0.5)
    h = ev.Bandwidths()
    want = W.ref_weighted_factors(c.table, c.nfields, D, c.lower, c.upper, h, m, 0.5)
    lam = ev.LocalFactors()
    rel = float(np.max(np.abs(lam - want) / want))
    print("D=%d N=%d: lambda %.3g .. %.3g, worst relative error %.3g" % (D, N, lam.min(), lam.max(), rel))
    assert rel <= 1e-11 and lam.min() < 0.95 and lam.max() > 1.05
    got = run(ev, c)
    ref = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                             dataset=c.dataset, alpha=0.5)
    assert got["norm"] == ref.norm
    ok, ratio, _ = compare(got["values"], ref)
    print("  values %.3g x the bound" % ratio)
    assert ok
    for plant in W.PLANTS[:3]:
        bad = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                                 dataset=c.dataset, alpha=0.5, plant=plant)
        assert not compare(got["values"], bad)[0], plant
    ev.close()


# ------------------------------------------------------------------ 4. cutoff
@pytest.mark.parametrize("alpha", [0.0, 0.5], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("D,N,E", [W.SHAPES[5], W.SHAPES[4], W.SHAPES[2]])
def test_cutoff(D, N, E, alpha):
    R = 4.0
    c = W.case(D, N, E)
    c.scale = c.scale * 0.25                     # (bandwidths narrow enough for the radius to cull)
    m = W.small_multiplicities(c)
    # the second tile of the cutoff's spatial order (a sort in one observable, the Morton order of a cell grid in more)
    # all zero: at N = 257 that tile holds one row
    order = W.spatial_order(c.table, D, c.lower, c.upper)
    m[order[TILE:2 * TILE]] = 0
    ev = evaluator(c, m, alpha)
    ev.SetCutoff(R)
    got = run(ev, c)
    visited, possible = ev.CutoffStats()
    tiles, waves = ev.CutoffBoxes()
    live = np.isfinite(waves[:, 0])
    v = replay_visits(D, tiles, waves, R)
    assert not v[~live].any() and possible == int(live.sum()) * len(tiles)
    print("D=%d N=%d %s: visited %d of %d" % (D, N, "adaptive" if alpha else "fixed", visited, possible))
    assert visited == int(v.sum())
    # the all-zero tile's box is empty and no wave visits it; a tile's box is empty exactly when none of its rows is live
    # (inside the domain after the systematics, m > 0) -- besides the second only a last tile of one such row can be
    assert np.all(tiles[1, :D] == np.inf) and np.all(tiles[1, 4:4 + D] == -np.inf) and not v[:, 1].any()
    moved = ref_transform(c.table, c.nfields, c.systs, W.PARAMS)[:, :D]
    live_row = np.all((moved >= c.lower) & (moved < c.upper), axis=1) & (m > 0)
    empty = [not live_row[order[t * TILE:(t + 1) * TILE]].any() for t in range(len(tiles))]
    assert empty[1] and not empty[0] and sum(empty) <= 2
    assert np.array_equal(np.all(tiles[:, :D] == np.inf, axis=1), empty)
    assert not v[:, empty].any() and 0 < visited < possible
    ref = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                             dataset=c.dataset, alpha=alpha, R=R)
    assert got["norm"] == ref.norm
    val = got["values"].astype(np.float64)
    assert np.array_equal(np.isnan(val), np.isnan(ref.full))
    ok = ~np.isnan(ref.full)
    worst = float(np.max(np.maximum(val[ok] - ref.full[ok], ref.kept[ok] - val[ok]) / ref.bound[ok]))
    print("  worst excess / bound %.3g" % worst)
    assert worst <= 1.0
    ev.close()


# ------------------------------------------------------------------ 5. projection
@pytest.mark.parametrize("alpha", [0.0, 0.5], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("D,N,E", W.SHAPES[:5])
def test_projection(D, N, E, alpha):
    c = W.case(D, N, E)
    m = W.small_multiplicities(c)
    ev = evaluator(c, m, alpha)
    run(ev, c, do_eval_pdf=False)
    h, lam = ev.Bandwidths(), ev.LocalFactors()
    for obs in range(D):
        for nbins in (1, 13, 70):
            got = ev.Project(obs, nbins)
            want = W.ref_weighted_marginal(c.table, c.nfields, D, c.lower, c.upper, h, lam, c.systs, W.PARAMS, m, obs, nbins)
            assert np.max(np.abs(got - want)) <= 1e-11 and abs(got.sum() - 1.0) <= 1e-11
            if nbins > 1:
                for plant in ("sum_unweighted", "norm_unweighted"):
                    bad = W.ref_weighted_marginal(c.table, c.nfields, D, c.lower, c.upper, h, lam, c.systs, W.PARAMS, m,
                                                  obs, nbins, plant=plant)
                    assert np.max(np.abs(got - bad)) > 1e-6, plant
    ev.close()


# ------------------------------------------------------------------ 6. a shared evaluator
@pytest.mark.parametrize("alpha", [0.0, 0.5], ids=["fixed", "adaptive"])
def test_shared_evaluator_returns_its_bases_bytes(alpha):
    D, N, E = W.SHAPES[4]
    c = W.case(D, N, E)
    m = W.small_multiplicities(c)
    base = evaluator(c, m, alpha)
    twin = pdfz.EvalKernel.Shared(base)
    assert twin.HasSampleMultiplicities() and twin.SampleTotal() == base.SampleTotal() == int(m.sum())
    assert np.array_equal(twin.SampleMultiplicities(), m) and twin.EffectiveSamples() == base.EffectiveSamples()
    a, b = run(base, c), run(twin, c)
    assert a["norm"] == b["norm"] and same_bytes(a["values"], b["values"])
    assert same_bytes(base.RandomSample(400, SEED), twin.RandomSample(400, SEED))
    assert same_bytes(base.Project(0, 9), twin.Project(0, 9))
    base.close()
    c2 = run(twin, c)                            # (the column outlives the base)
    assert same_bytes(a["values"], c2["values"])
    twin.close()


# ------------------------------------------------------------------ refusals
def test_refusals():
    D, N, E = W.SHAPES[1]
    c = W.case(D, N, E)
    with pytest.raises(pdfz.Error, match="255 given for 256 rows"):
        evaluator(c, np.ones(N - 1, np.uint32))
    with pytest.raises(pdfz.Error, match="exceeds 4294967295"):
        evaluator(c, np.full(N, 2 ** 25, np.uint32))
    ev = evaluator(c, W.small_multiplicities(c))
    with pytest.raises(capi.SxmcError, match="cross-validation of an evaluator with sample multiplicities is not built"):
        ev.SelectBandwidthScale()
    with pytest.raises(capi.SxmcError, match="cross-validation of an evaluator with sample multiplicities is not built"):
        ev.CvScores([ev.Bandwidths()])
    ev.close()
