"""CPU: the reference of the cutoff tests checks itself (tests/kde_cutoff_reference.py) -- the envelope is ordered and
collapses onto the contract value at R = +infinity, agrees with the existing references' values, and its negative
control (the sum that also drops the pairs of q' in [0.8 qcut, qcut)) lies outside it at R = 3 on the very inputs the
GPU tests use; the numpy replay of the visit test on constructed boxes; the adaptive clip table clips at both ends.
For the shapes at which a workgroup walks many tiles (tests/test_gpu_kde_cutoff_splits.py): the control on each
regime's strided points against a smaller table of the same generator, the strided places themselves, and the local
factors passed to the reference as an input."""
import math

import numpy as np
import pytest

from tests.kde_adaptive_reference import ref_kde_adaptive, ref_local_factors
from tests.kde_cutoff_reference import (PAIRS_PER_CASE, PARAMS, REGIMES, SUBSAMPLE, clip_table, cutoff_points,
                                        cutoff_systs, cutoff_table, inside_envelope, qcut_f32, qcut_of, ref_cutoff, regime_inputs,
                                        replay_visits, strided)
from tests.kde_reference import ref_kde


@pytest.mark.parametrize("alpha", [0.0, 0.5], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_envelope_and_its_negative_control(D, alpha):
    rng = np.random.default_rng(8000 + D)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    pts = cutoff_points(D, 300, rng, lower, upper)
    scale, systs = [0.5] * D, cutoff_systs(D)
    args = (samples, nf, D, lower, upper, scale, alpha, systs, PARAMS, pts)
    old = (ref_kde_adaptive(*args) if alpha > 0 else
           ref_kde(samples, nf, D, lower, upper, scale, systs, PARAMS, pts))
    for R in (3.0, 6.0, math.inf):
        ref = ref_cutoff(*args, R)
        ok = ~np.isnan(ref.full)
        assert ref.norm == old.norm and 500 < ref.norm < 1000
        assert np.array_equal(np.isnan(ref.full), np.isnan(old.values)) and 0 < (~ok).sum() < 100
        assert np.allclose(ref.full[ok], old.values[ok], rtol=1e-12, atol=0)
        assert np.all(ref.bound[ok] >= old.bound[ok] * 0.9999999)       # (256 S0 covers any row order)
        assert np.all(ref.kept[ok] <= ref.full[ok]) and np.all(ref.culled[ok] <= ref.kept[ok])
        assert inside_envelope(ref.full, ref)[0] and inside_envelope(ref.kept, ref)[0]
        if math.isinf(R):
            assert np.array_equal(ref.kept[ok], ref.full[ok])
        else:
            assert np.any(ref.kept[ok] < ref.full[ok])                  # (something is dropped: the envelope has width)
        if R == 3.0:
            bad, excess = inside_envelope(ref.culled, ref)
            print("D=%d alpha=%g: the over-culled sum is outside by %.3g x the bound" % (D, alpha, excess))
            assert not bad and excess > 10
        # a value with a NaN in the wrong place, or above the full sum, fails
        wrong = ref.full.copy()
        wrong[np.flatnonzero(ok)[0]] = np.nan
        assert not inside_envelope(wrong, ref)[0]
        assert not inside_envelope(ref.full + 3 * ref.bound, ref)[0]


def test_qcut():
    assert qcut_of(0.0) == 0.0 and math.isinf(qcut_of(math.inf)) and abs(qcut_of(15.0) - 162.303) < 1e-3
    for R in (1.0, 3.0, 4.0, 6.0, 15.0):
        f = qcut_f32(R)
        assert f.dtype == np.float32 and float(f) >= qcut_of(R) > float(np.nextafter(f, np.float32(0)))
    assert np.isinf(qcut_f32(math.inf))


def test_replay_of_the_visit_test():
    inf = np.inf
    tiles = np.array([[13, 0, 0, 0, 20, 0, 0, 0, 1], [13, 0, 0, 0, 20, 0, 0, 0, 0.25],
                      [inf, inf, inf, inf, -inf, -inf, -inf, -inf, 1], [5, 0, 0, 0, 6, 0, 0, 0, 1]], np.float32)
    waves = np.array([[0, 0, 0, 0, 10, 0, 0, 0], [inf, inf, inf, inf, -inf, -inf, -inf, -inf]], np.float32)
    R3 = math.sqrt(9.0 / 0.72134752044448170)                           # qcut about 9: the gap of 3 sits on it
    v = replay_visits(1, tiles, waves, R3 * 1.001)
    assert v.tolist() == [[True, True, False, True], [False] * 4]
    v = replay_visits(1, tiles, waves, R3 * 0.999)
    assert v.tolist() == [[False, True, False, True], [False] * 4]
    assert replay_visits(1, tiles, waves, math.inf).tolist() == [[True, True, False, True], [False] * 4]
    # two observables: the gaps add
    t2 = np.array([[13, 14, 0, 0, 20, 20, 0, 0, 1]], np.float32)
    w2 = np.array([[0, 0, 0, 0, 10, 10, 0, 0]], np.float32)
    assert replay_visits(2, t2, w2, math.sqrt(25.01 / 0.72134752044448170)).tolist() == [[True]]
    assert replay_visits(2, t2, w2, math.sqrt(24.99 / 0.72134752044448170)).tolist() == [[False]]


def test_clip_table_clips_at_both_ends():
    samples, nf, lower, upper = clip_table()
    lam = ref_local_factors(samples, nf, 2, lower, upper, [0.3, 0.3], 1.0)
    low, high = float(np.mean(lam == 0.1)), float(np.mean(lam == 10.0))
    print("rows at lambda 0.1: %.1f %%, at 10: %.1f %%" % (100 * low, 100 * high))
    assert low >= 0.01 and high >= 0.01 and 1 - low - high >= 0.5


SPLIT_CASES = [(name, D, 0.0) for name in ("A", "B1", "B2", "C1") for D in (1, 4)] + [("A'", 2, 0.0), ("C2", 2, 0.0),
                                                                                      ("A", 2, 0.5), ("B2", 2, 0.5)]


@pytest.mark.parametrize("name,D,alpha", SPLIT_CASES, ids=["%s-D%d-%g" % c for c in SPLIT_CASES])
def test_the_control_on_the_strided_points_of_a_regime(name, D, alpha):
    """The points are the GPU test's own; the table is 2000 rows of its generator (the full one costs seconds a case,
    and the GPU test asserts the control on it as well)."""
    npts, nrows = REGIMES[name]
    samples, nf, lower, upper, pts = regime_inputs(name, D, rows=2000)
    assert pts.size == npts * (D + 1) and samples.size == 2000 * nf
    idx = strided(npts, nrows)
    sub = pts.reshape(npts, D + 1)[idx]
    ref = ref_cutoff(samples, nf, D, lower, upper, [0.5] * D, alpha, cutoff_systs(D), PARAMS, sub.ravel(), 3.0)
    ok = ~np.isnan(ref.full)
    assert ok.sum() > 0.5 * len(idx) and np.isnan(ref.full[1]) and ref.full[2] == 0.0     # (the special points are in)
    assert np.any(ref.kept[ok] < ref.full[ok]) and inside_envelope(ref.kept, ref)[0]
    bad, excess = inside_envelope(ref.culled, ref)
    print("%s D=%d alpha=%g: the over-culled sum is outside by %.3g x the bound" % (name, D, alpha, excess))
    assert not bad and excess > 10


def test_the_strided_places_span_the_points():
    assert strided(0).tolist() == [] and strided(7).tolist() == list(range(7))
    assert strided(SUBSAMPLE).tolist() == list(range(SUBSAMPLE))
    for npts, nrows in list(REGIMES.values()) + [(40000, 4000), (60000, 4000), (SUBSAMPLE + 1, 0)]:
        idx = strided(npts, nrows)
        gaps = np.diff(idx)
        cap = int(min(SUBSAMPLE, max(128, PAIRS_PER_CASE // max(nrows, 1))))
        assert cap // 2 <= len(idx) <= cap and idx[0] == 0 and idx[-1] == npts - 1 and np.all(gaps > 0)
        assert gaps.max() <= -(-npts // (cap - 3))                                # (no stretch of the array is left out)
        # 64 points to a wave: the places fall in as many waves as there are strided places, or in every wave
        assert len(np.unique(idx // 64)) >= min(len(idx) - 3, -(-npts // 64))


@pytest.mark.parametrize("D", [1, 2])
def test_local_factors_as_an_input_of_the_reference(D):
    rng = np.random.default_rng(8000 + D)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    pts = cutoff_points(D, 300, rng, lower, upper)
    args = (samples, nf, D, lower, upper, [0.5] * D, 0.5, cutoff_systs(D), PARAMS, pts, 3.0)
    lam = ref_local_factors(samples, nf, D, lower, upper, [0.5] * D, 0.5)
    a, b = ref_cutoff(*args), ref_cutoff(*args, lam=lam)
    for f in ("full", "kept", "bound", "culled"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    assert a.norm == b.norm and a.c_max == b.c_max
    # ... and they are read: other factors, other values; none at sensitivity 0
    c = ref_cutoff(*args, lam=1.5 * lam)
    assert c.full.tobytes() != a.full.tobytes()
    fixed = args[:6] + (0.0,) + args[7:]
    assert ref_cutoff(*fixed, lam=lam).full.tobytes() == ref_cutoff(*fixed).full.tobytes()
