"""GPU tests of pdfz::EvalKernel's bandwidth cross-validation (sxmc_kde_cv_scores, sxmc_kde_cv_select, CrossValidated)
against the f64 reference (tests/kde_cv_reference.py, which derives the bound the scores are held to):

* scores in 1-4 D, at the sizes where the split over workgroups changes, on tables with rows outside the domain between
  rows inside, a row one float below `upper`, a row on `lower` and duplicated rows, with 1, 21 and 32 candidates, one
  of them small enough to score -inf: |device - reference| <= 2 * bound (the reference's own f64 arithmetic sits within
  the same bound);
* determinism: two calls and a shared evaluator give the same bytes;
* max_rows: the scores of exactly the subset the host header names;
* the search: the choices, edges, rows and scans of the reference on the gap-checked cases
  (tests/test_kde_cv_reference_cpu.py asserts the gaps);
* CrossValidated(...) against an evaluator constructed with the chosen scales typed in, fixed and adaptive, as bytes."""
import math

import numpy as np
import pytest

from sxmc_amd import pdfz
from tests import kde_cv_reference as cv
from tests.kde_adaptive_reference import ref_local_factors
from tests.kde_reference import ref_bandwidths
from tests.test_gpu_kde import gpu_kde

pytestmark = pytest.mark.gpu

GRAIN = cv.CV_GRAIN
# one past the largest m that still takes the smallest per_split (with one candidate: all 16 splits are allowed)
PAST_SMALLEST = cv.CV_SPLITS * GRAIN + 1


def evaluator(x, D, lower, upper, scale=None, alpha=0.0):
    return pdfz.EvalKernel(x.ravel(), x.shape[1], D, list(lower), list(upper), scale or [1.0] * D,
                           bandwidth_sensitivity=alpha)


def check_scores(label, ev, x, D, lower, upper, mult, max_rows=0):
    """The device's scores of the candidates mult [K, D] (multipliers of sigma m^(-1/(D+4))) against the reference's."""
    rows, n, sigma = cv.scored_rows(x.ravel(), x.shape[1], D, lower, upper, max_rows)
    h = cv.candidates(mult, sigma, len(rows))
    want, bound = cv.scores(rows, lower, upper, h)
    got, m = ev.CvScores(h, max_rows)
    assert m == len(rows) and got.shape == want.shape and got.dtype == np.float64
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite) and np.all(got[~finite] == -math.inf), (label, got, want)
    err = np.abs(got[finite] - want[finite])
    share = float(np.max(err / (2 * bound[finite]))) if finite.any() else 0.0
    print("%s: m=%d K=%d split=%s worst error %.3g, allowed %.3g (share %.3g)"
          % (label, m, len(h), cv.split(m, len(h)), err.max(initial=0.0), 2 * bound[finite].max(initial=0.0), share))
    assert np.all(err <= 2 * bound[finite]), (label, err, bound)
    return got


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_scores_in_every_dimension(D):
    x, lower, upper = cv.table_with_inside(100 + D, GRAIN + 1, D, nfields=D + 1)
    assert len(x) > GRAIN + 1                              # rows outside the domain lie between rows inside
    ev = evaluator(x, D, lower, upper)
    g = cv.grid(0.125, 4.0, 21)
    mult = np.tile(g[:, None], (1, D))
    mult[:, D - 1] = g[::-1]                               # (not one multiplier on every observable)
    got = check_scores("D=%d" % D, ev, x, D, lower, upper, mult)
    assert np.isfinite(got).sum() >= 20 and len(set(got)) == 21   # (1/8 of Scott's rule isolates a row in 4-D)
    ev.close()


@pytest.mark.parametrize("m", [2, 3, GRAIN - 1, GRAIN, GRAIN + 1, 2 * GRAIN + 1])
def test_scores_at_the_split_sizes(m):
    x, lower, upper = cv.table_with_inside(200 + m, m, 2)
    ev = evaluator(x, 2, lower, upper)
    check_scores("m=%d" % m, ev, x, 2, lower, upper, [[0.5, 0.5], [1.0, 2.0], [3.0, 0.7]])
    ev.close()


def test_scores_one_past_the_largest_size_with_the_smallest_split():
    m = PAST_SMALLEST
    assert cv.split(m - 1, 1) == (GRAIN, cv.CV_SPLITS) and cv.split(m, 1) == (2 * GRAIN, (m + 2 * GRAIN - 1) // (2 * GRAIN))
    x, lower, upper = cv.table_with_inside(300, m, 1)
    ev = evaluator(x, 1, lower, upper)
    check_scores("m=%d, one candidate" % m, ev, x, 1, lower, upper, [[0.8]])
    ev.close()


def test_thirty_two_candidates_with_one_that_scores_minus_infinity():
    x, lower, upper = cv.table_with_inside(400, 300, 2)
    ev = evaluator(x, 2, lower, upper)
    mult = np.tile(cv.grid(0.2, 5.0, 32)[:, None], (1, 2))
    mult[7] = 1e-4                                         # no neighbour within exp's range: -inf beside finite scores
    got = check_scores("K=32", ev, x, 2, lower, upper, mult)
    assert got[7] == -math.inf and np.isfinite(np.delete(got, 7)).all()
    # the same candidates one at a time (K = 1: another instantiation) within the bound of the same reference
    for c in (0, 7, 31):
        one = check_scores("K=1, candidate %d" % c, ev, x, 2, lower, upper, mult[c:c + 1])
        assert (one[0] == got[c]) or abs(one[0] - got[c]) < 1e-12
    ev.close()


def test_two_calls_and_a_shared_evaluator_give_the_same_bytes():
    x, lower, upper = cv.table_with_inside(500, 2 * GRAIN + 40, 3)
    ev = evaluator(x, 3, lower, upper)
    before = ev.Bandwidths()
    _, _, sigma = cv.scored_rows(x.ravel(), 3, 3, lower, upper)
    h = cv.candidates(np.tile(cv.grid(0.25, 4.0, 9)[:, None], (1, 3)), sigma, 2 * GRAIN + 40)
    a, m = ev.CvScores(h)
    b, _ = ev.CvScores(h)
    shared = pdfz.EvalKernel.Shared(ev)
    c, mc = shared.CvScores(h)
    assert m == mc == 2 * GRAIN + 40 and a.tobytes() == b.tobytes() == c.tobytes()
    r1, r2 = ev.SelectBandwidthScale(pdfz.CvOptions(0.25, 4.0, 9, True, 0)), shared.SelectBandwidthScale(
        pdfz.CvOptions(0.25, 4.0, 9, True, 0))
    assert r1.scale.tobytes() == r2.scale.tobytes() and r1.score == r2.score
    for s1, s2 in zip(r1.scans, r2.scans):
        assert s1.scores.tobytes() == s2.scores.tobytes()
    # the evaluator's own bandwidths did not move, and an adaptive evaluator scores the same global stage
    assert ev.Bandwidths().tobytes() == before.tobytes()
    ad = evaluator(x, 3, lower, upper, alpha=0.5)
    assert ad.CvScores(h)[0].tobytes() == a.tobytes()
    for e in (ev, shared, ad):
        e.close()


@pytest.mark.parametrize("max_rows", [GRAIN - 1, 100, 37])
def test_max_rows_scores_the_subset_the_header_names(max_rows):
    x, lower, upper = cv.table_with_inside(600, GRAIN, 2, nfields=3)      # n = max_rows + 1, and n >> max_rows
    ev = evaluator(x, 2, lower, upper)
    rows, n, _ = cv.scored_rows(x.ravel(), 3, 2, lower, upper, max_rows)
    assert n == GRAIN and len(rows) == len(cv.subset(n, max_rows)) <= max_rows
    check_scores("max_rows=%d" % max_rows, ev, x, 2, lower, upper, [[0.5, 1.0], [1.0, 1.0], [2.0, 0.5]], max_rows)
    ev.close()


# ------------------------------------------------------------------ the search
@pytest.mark.parametrize("name", sorted(cv.selection_cases()))
def test_search_equals_the_reference(name):
    x, D, lower, upper, o = cv.selection_cases()[name]
    want = cv.select(x.ravel(), x.shape[1], D, lower, upper, o)
    ev = evaluator(x, D, lower, upper)
    got = ev.SelectBandwidthScale(pdfz.CvOptions(o.lo, o.hi, o.steps, o.per_observable, o.max_rows))
    print("%s: chose %s (reference %s), score %.9g (reference %.9g), at s = 1 %.9g, rows %d"
          % (name, got.scale, want["scale"], got.score, want["score"], got.score_at_one, got.rows_used))
    assert np.array_equal(got.scale, want["scale"]) and got.at_edge == list(want["at_edge"])
    assert got.rows_used == want["rows_used"] and len(got.scans) == len(want["scans"])
    for s, w in zip(got.scans, want["scans"]):
        assert s.observable == w["observable"] and s.chosen == w["chosen"] and np.array_equal(s.grid, w["grid"])
        # (the gap condition's figure: a score error below it cannot move a choice; the scores themselves are held to
        #  the derived bound by the tests above)
        fin = np.isfinite(w["scores"])
        assert np.array_equal(np.isfinite(s.scores), fin) and np.all(np.abs(s.scores[fin] - w["scores"][fin]) < 1e-9)
    assert abs(got.score - want["score"]) < 1e-9
    if math.isnan(want["score_at_one"]):
        assert math.isnan(got.score_at_one)
    else:
        assert abs(got.score_at_one - want["score_at_one"]) < 1e-9
    best = [s.scores[s.chosen] for s in got.scans]
    assert all(b >= a for a, b in zip(best, best[1:]))
    assert np.array_equal(ev.BandwidthScale(), np.ones(D))             # the evaluator keeps what it was built with
    ev.close()


def test_search_refuses_what_it_cannot_do():
    x, lower, upper = cv.table_with_inside(700, 50, 1)
    ev = evaluator(x, 1, lower, upper)
    for o, msg in ((pdfz.CvOptions(steps=0), "steps must be between 1 and 32"),
                   (pdfz.CvOptions(steps=33), "steps must be between 1 and 32"),
                   (pdfz.CvOptions(lo=2.0, hi=1.0), "0 < lo <= hi"),
                   (pdfz.CvOptions(lo=1e-7, hi=1e-6, steps=3, max_rows=0), "no finite score"),
                   (pdfz.CvOptions(max_rows=1), "at least 2 rows")):
        with pytest.raises(pdfz.Error) as e:
            ev.SelectBandwidthScale(o)
        assert msg in e.value.msg
    for bad, msg in (([[0.0]], "positive and finite"), ([[math.nan]], "positive and finite"),
                     ([[1.0]] * 33, "between 1 and 32")):
        with pytest.raises(pdfz.Error) as e:
            ev.CvScores(bad)
        assert msg in e.value.msg
    ev.close()


# ------------------------------------------------------------------ the factory
@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_cross_validated_is_the_evaluator_with_the_scales_typed_in(alpha):
    x, D, lower, upper, o = cv.selection_cases()["blob_2d_per_observable"]
    want = cv.select(x.ravel(), x.shape[1], D, lower, upper, o)
    opts = pdfz.CvOptions(o.lo, o.hi, o.steps, o.per_observable, o.max_rows)
    ev = pdfz.EvalKernel.CrossValidated(x.ravel(), x.shape[1], D, list(lower), list(upper), opts,
                                        bandwidth_sensitivity=alpha)
    assert np.array_equal(ev.BandwidthScale(), want["scale"]) and len(set(want["scale"])) == 2
    assert np.array_equal(ev.CvReport().scale, want["scale"]) and ev.CvReport().rows_used == want["rows_used"]
    typed = evaluator(x, D, lower, upper, list(want["scale"]), alpha)
    assert typed.CvReport() is None and ev.BandwidthSensitivity() == alpha
    assert ev.Bandwidths().tobytes() == typed.Bandwidths().tobytes()
    assert np.allclose(ev.Bandwidths(), ref_bandwidths(x.ravel(), x.shape[1], D, lower, upper, want["scale"]),
                       rtol=1e-13, atol=0)
    assert ev.LocalFactors().tobytes() == typed.LocalFactors().tobytes()
    if alpha:
        lam = ref_local_factors(x.ravel(), x.shape[1], D, lower, upper, list(want["scale"]), alpha)
        assert np.max(np.abs(ev.LocalFactors() - lam) / lam) <= 1e-11 and lam.min() < 0.9
    rng = np.random.default_rng(9)
    pts = np.concatenate([rng.uniform(-5, 5, (300, D)), np.zeros((300, 1))], axis=1).astype(np.float32).ravel()
    a = gpu_kde(None, None, D, lower, upper, None, (), {}, pts, ev=ev)
    b = gpu_kde(None, None, D, lower, upper, None, (), {}, pts, ev=typed)
    assert a["norm"] == b["norm"] and a["values"].tobytes() == b["values"].tobytes()
    shared = pdfz.EvalKernel.Shared(ev)
    assert np.array_equal(shared.BandwidthScale(), want["scale"]) and shared.CvReport() is ev.CvReport()
    assert shared.Bandwidths().tobytes() == ev.Bandwidths().tobytes()
    for e in (ev, typed, shared):
        e.close()
