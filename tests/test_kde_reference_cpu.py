"""CPU: the kernel-density reference (tests/kde_reference.py) checked against mpmath (truncation masses at the edges and
at extreme bandwidths, Scott's rule, pdf values), and its error bound checked both ways on an emulation of the kernels'
f32 arithmetic: the emulation stays inside the bound in 1-4 D, and each planted error (bandwidth, untruncated weights,
swapped observables, norm) takes the comparison outside it."""
import math

import numpy as np
import pytest

from tests.kde_reference import (PLANTS, check_power, check_values, emulate_kernel, ref_bandwidths, ref_kde,
                                 truncation_mass)


def mp_mass(mp, s, h, lo, hi):
    """Phi((hi - s)/h) - Phi((lo - s)/h) at 60 digits, every input taken exactly."""
    s, h, lo, hi = (mp.mpf(float(v)) for v in (s, h, lo, hi))
    return (mp.erfc((s - hi) / (h * mp.sqrt(2))) - mp.erfc((s - lo) / (h * mp.sqrt(2)))) / 2


@pytest.mark.parametrize("width_over_h", [1e-3, 1.0, 8.0, 1e3])
def test_truncation_mass_against_mpmath(width_over_h):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    lo, hi = 2.0, 5.0
    h = (hi - lo) / width_over_h
    top = float(np.nextafter(np.float32(hi), np.float32(0)))
    for s in (lo, top, 0.5 * (lo + hi), lo + 1e-3 * (hi - lo), float(np.float32(lo + 0.999 * (hi - lo)))):
        got = float(truncation_mass(np.array([[s]]), [h], [lo], [hi])[0])
        want = mp_mass(mp, s, h, lo, hi)
        rel = abs(got - float(want)) / float(want)
        inv = abs(1.0 / got - float(1 / want)) * float(want)
        print("w/h %g, s %.9g: mass %.17g, relative error %.2g (1/w %.2g)" % (width_over_h, s, got, rel, inv))
        # two erfc in f64: each good to a few ulp of its value, so the mass to a few ulp of the larger one
        assert rel <= 1e-13 * max(1.0, float(mp.erfc(0) / (2 * want))) and inv <= 1e-13 * max(1.0, 1 / float(want))


def test_scott_bandwidth_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rng = np.random.default_rng(1)
    x = np.stack([rng.normal(1.0, 0.3, 700), rng.uniform(-5, 5, 700), rng.exponential(2.0, 700)], axis=1)
    x = x.astype(np.float32)
    lower, upper = np.array([0.0, -4.0, 0.0]), np.array([2.0, 4.0, 6.0])
    h = ref_bandwidths(x.ravel(), 3, 3, lower, upper, [1.0, 0.5, 2.0])
    inside = np.all((x.astype(np.float64) >= lower) & (x.astype(np.float64) < upper), axis=1)
    n = int(inside.sum())
    for d, sc in enumerate((1.0, 0.5, 2.0)):
        v = [mp.mpf(float(a)) for a in x[inside, d]]
        mean = mp.fsum(v) / n
        sigma = mp.sqrt(mp.fsum((a - mean) ** 2 for a in v) / (n - 1))
        want = sc * sigma * mp.power(n, mp.mpf(-1) / 7)
        assert abs(h[d] - float(want)) <= 1e-13 * float(want)


def test_pdf_values_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rng = np.random.default_rng(2)
    s = np.stack([rng.normal(0.5, 0.2, 40), rng.normal(-1.0, 0.5, 40)], axis=1).astype(np.float32)
    lower, upper = [0.0, -2.0], [1.0, 0.0]
    pts = np.array([[0.5, -1.0, 0], [0.01, -1.99, 0], [0.97, -0.02, 0], [0.3, -0.5, 0]], np.float32)
    ref = ref_kde(s.ravel(), 2, 2, lower, upper, [1.0, 1.0], [], {}, pts.ravel())
    ins = [r for r in s.astype(np.float64) if all(lower[d] <= r[d] < upper[d] for d in range(2))]
    h = [mp.mpf(float(v)) for v in ref.h]
    assert ref.norm == len(ins)
    for i, p in enumerate(pts):
        tot = mp.mpf(0)
        for r in ins:
            term = mp.mpf(1)
            for d in range(2):
                z = (mp.mpf(float(p[d])) - mp.mpf(float(r[d]))) / h[d]
                mass = mp_mass(mp, r[d], h[d], lower[d], upper[d])
                term *= mp.exp(-z * z / 2) / (mp.sqrt(2 * mp.pi) * h[d] * mass)
            tot += term
        want = float(tot / len(ins))
        assert abs(ref.values[i] - want) <= 1e-13 * want, (i, ref.values[i], want)


def separable_case(D, extra, n, npts, rng):
    """D observables + `extra` fields, systematics of all four kinds, in-domain points of data set 0 and 1, points
    outside."""
    lower, upper = np.linspace(-1.0, 0.5, D), np.linspace(2.0, 4.0, D)
    cols = [rng.uniform(lower[d] - 0.1, upper[d] + 0.1, n) for d in range(D)]
    cols += [rng.normal(1.0, 0.3, n) for _ in range(extra)]
    samples = np.stack(cols, axis=1).astype(np.float32)
    systs = [dict(type="shift", obs=0, pars=[0, 1]), dict(type="scale", obs=D - 1, pars=[2])]
    if D > 1:
        systs.append(dict(type="ctscale", obs=1, pars=[3]))
    if extra:
        systs.append(dict(type="resolution_scale", obs=0, true_obs=D, pars=[4]))
    params = {0: 0.02, 1: -0.01, 2: 0.03, 3: -0.02, 4: 0.05}
    p = np.concatenate([rng.uniform(lower - 0.05, upper + 0.05, (npts, D)),
                        (rng.random((npts, 1)) < 0.1).astype(np.float64)], axis=1).astype(np.float32)
    return samples.ravel(), D + extra, lower, upper, systs, params, p.ravel()


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_bound_holds_for_the_emulated_kernel_and_planted_errors_break_it(D):
    rng = np.random.default_rng(10 + D)
    samples, nf, lower, upper, systs, params, pts = separable_case(D, 1, 700, 300, rng)
    args = (samples, nf, D, lower, upper, [0.8] * D, systs, params, pts)
    got, norm = emulate_kernel(*args)
    ref = ref_kde(*args)
    assert norm == ref.norm and ref.norm < 700
    check_values(got, ref, "emulated %d-D" % D)
    plants = [p for p in PLANTS if p != "swap" or D >= 2]
    check_power(got, lambda p: ref_kde(*args, plant=p), plants, "emulated %d-D" % D)


def test_bound_holds_where_coordinates_lie_far_from_lower():
    # data 300 bandwidths from lower: the f32 coordinates dominate the bound and the emulation's error
    rng = np.random.default_rng(20)
    s = rng.normal(300.0, 1.0, 600).astype(np.float32)
    pts = np.stack([rng.uniform(297.0, 303.0, 400), np.zeros(400)], axis=1).astype(np.float32).ravel()
    args = (s, 1, 1, [0.0], [310.0], [1.0], [], {}, pts)
    got, _ = emulate_kernel(*args)
    ref = ref_kde(*args)
    assert ref.c_max > 500
    ratio = check_values(got, ref, "far from lower")
    assert ratio > 0.01        # (the bound follows the error there: not loose by orders of magnitude)


def test_reference_special_points():
    s = np.array([0.2, 0.4, 0.6], np.float32)
    pts = np.array([[0.5, 0], [0.5, 1], [1.0, 0], [np.nan, 0], [-1e-9, 0]], np.float32).ravel()
    ref = ref_kde(s, 1, 1, [0.0], [1.0], [1.0], [], {}, pts)
    v = ref.values
    assert v[0] > 0 and v[1] == 0 and all(math.isnan(a) for a in v[2:])
    gone = ref_kde(s, 1, 1, [0.0], [1.0], [1.0], [dict(type="shift", obs=0, pars=[0])], {0: 2.0}, pts)
    assert gone.norm == 0 and math.isnan(gone.values[0]) and gone.values[1] == 0
