"""CPU: the reference of the cutoff tests checks itself (tests/kde_cutoff_reference.py) -- the envelope is ordered and
collapses onto the contract value at R = +infinity, agrees with the existing references' values, and its negative
control (the sum that also drops the pairs of q' in [0.8 qcut, qcut)) lies outside it at R = 3 on the very inputs the
GPU tests use; the numpy replay of the visit test on constructed boxes; the adaptive clip table clips at both ends."""
import math

import numpy as np
import pytest

from tests.kde_adaptive_reference import ref_kde_adaptive, ref_local_factors
from tests.kde_cutoff_reference import (PARAMS, clip_table, cutoff_points, cutoff_systs, cutoff_table, inside_envelope,
                                        qcut_f32, qcut_of, ref_cutoff, replay_visits)
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
