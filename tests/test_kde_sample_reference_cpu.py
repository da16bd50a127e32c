"""CPU: the numpy replay of the kernel-density event sampler (tests/kde_sample_reference.py), the cases the GPU test
(tests/test_gpu_kde_sample_replay.py) holds the device to, and whether the comparison can see a wrong sampler.

* The replay obeys the law: KS against the exact mixture CDF on the case of test_law_1d_truncation_matters.
* The replay is accurate: xd against 60-digit arithmetic (mpmath) within 64 x 2^-53 max(|xd|, hw) on 200 draws over
  h = 0.003, 0.3 and 5 on [0.1, 10), centres at both ends, extreme words included (measured: 10.8).
* Every case keeps within the cap of 1e-3 ambiguous events (a condition on the inputs, not a tolerance) and reaches the
  path it is there for (check_replay).
* Negative controls: each variant changes more than 1 % of the events of some case, and the comparison of the GPU test
  fails on it.  Over the cases of the GPU test one_minus_p changes no event at all: the two forms of q differ by about
  1e-16 of the bandwidth, 1e-8 of a float step.  It shows in two other ways: it leaves the accuracy bound above by a
  factor of 1e5 and more in the far upper tail (words near 2^32), and it changes 2 % of the events of a replay-only
  control, a bandwidth ten million times a domain about zero, where floats are dense (and where delta exceeds the float
  spacing: nothing to hold a device to).  clamp_before_round changes 4 events in 100 000 at bandwidth_x0.001 and 3 %
  at bandwidth_x1e-06, a case added for it: samples within a few floats of the bounds under a bandwidth of one float.
* Edges of the replay: n = 1, no events, cuts equal to the domain, bottom / top at bounds that are floats and bounds
  that are not."""
import functools
import math

import mpmath
import numpy as np
import pytest

from tests import kde_sample_reference as R
from tests.kde_reference import ref_bandwidths

CASES = R.cases()


@functools.lru_cache(maxsize=None)
def replayed(name):
    """(h, lam, draw, n) of a case with the bandwidths and factors computed on the host."""
    c = CASES[name]
    h, lam = R.host_bandwidths(c), R.host_factors(c)
    d, n = c.replay(h, lam)
    return h, lam, d, n


def test_the_replay_obeys_the_law():
    rng = np.random.default_rng(21)
    lo, hi = 0.0, 10.0
    x = np.concatenate([np.clip(rng.normal(5.0, 1.2, 2730), 2.0, 8.0),
                        rng.uniform(0.0, 0.6, 683), rng.uniform(9.4, 10.0, 683)]).astype(np.float32)
    h = ref_bandwidths(x, 1, 1, np.array([lo]), np.array([hi]), [1.0])
    rows_c, idx, fragile = R.prepare(x[:, None], 1, 1, [lo], [hi], h)
    assert len(idx) == 4096
    N = 200000
    d = R.draw(rows_c, idx, np.ones(4096), h, [lo], [hi], N, 12345, fragile=fragile)
    ks = R.ks_distance(d["events"][:, 0].astype(np.float64), x.astype(np.float64), float(h[0]), lo, hi) * math.sqrt(N)
    print("KS D sqrt(N) = %.4f" % ks)
    assert ks < 1.95
    assert np.all(d["attempts"] == 1) and d["exhausted"] == 0 and np.all(d["events"][:, 1] == 0.0)
    # the centres the replay draws around are the samples, to the float rounding of the scaled coordinate
    s = lo + rows_c[:, 0].astype(np.float64) * (h[0] / R.KLOG)
    assert np.max(np.abs(s - x)) <= 2.0 ** -23 * 10.0


def exact_xd(c, factor, word, h, lower, upper):
    """point() in 60-digit arithmetic from the same f64 centre and bandwidth."""
    mp = mpmath.mp
    s = mp.mpf(lower + float(np.float32(c)) * (h / R.KLOG))
    hw = mp.mpf(h * factor)
    Phi = lambda z: mp.erfc(-z / mp.sqrt(2)) / 2   # noqa: E731
    a, b = (mp.mpf(lower) - s) / hw, (mp.mpf(upper) - s) / hw
    p = Phi(a) + (mp.mpf(int(word)) + mp.mpf(0.5)) / mp.mpf(2) ** 32 * (Phi(b) - Phi(a))
    z = mp.sqrt(2) * mp.erfinv(2 * p - 1) if p > mp.mpf("1e-20") else mp.findroot(lambda t: Phi(t) - p, a)
    return s + hw * z, hw


def accuracy_draws():
    """200 draws: h = 0.003, 0.3 and 5 on [0.1, 10), centres at both ends and inside, extreme and random words."""
    rng = np.random.default_rng(33)
    lower, upper = 0.1, 10.0
    out = []
    for h in (0.003, 0.3, 5.0):
        cs = R.KLOG / h
        centres = [0.1, 0.1 + 1e-7, 0.1 + 0.5 * h, 0.1 + 4 * h, 5.0, 10.0 - 4 * h, 10.0 - 0.5 * h, 10.0 - 1e-6]
        words = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
        for s in [min(max(s, lower), upper - 1e-6) for s in centres]:      # (a centre is a sample inside the domain)
            for w in words + [int(v) for v in rng.integers(0, 2 ** 32, 3)]:
                out.append((np.float32((s - lower) * cs), float(rng.choice([1.0, 0.37, 2.9])), w, h, lower, upper))
    return out[:200]


def worst_error(variant=None, only_upper_tail=False):
    mpmath.mp.dps = 60
    worst = 0.0
    for c, factor, w, h, lower, upper in accuracy_draws():
        if only_upper_tail and w < 2 ** 32 - 2:
            continue
        xd, hw = R.point(np.array([c]), factor, np.array([w], np.uint64), h, lower, upper, variant)
        want, _ = exact_xd(c, factor, w, h, lower, upper)
        err = abs(mpmath.mpf(float(xd[0])) - want) / (mpmath.mpf(2) ** -53 * max(abs(float(xd[0])), float(hw[0])))
        worst = max(worst, float(err))
    return worst


def test_the_replay_is_accurate():
    assert len(accuracy_draws()) == 200
    worst = worst_error()
    print("worst |xd - exact| = %.1f x 2^-53 max(|xd|, hw)" % worst)
    assert worst <= 64
    # the far upper tail is where the complement q = qb + (1 - u) m earns its keep
    lost = worst_error("one_minus_p", only_upper_tail=True)
    print("with q = 1 - p, words near 2^32: %.3g x 2^-53 max(|xd|, hw)" % lost)
    assert lost > 64 * 1000


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cases_keep_within_the_cap(name):
    h, lam, d, n = replayed(name)
    share = float(np.mean(R.excused(d)))
    print("%s: n = %d, h = %s, %.3g of the events ambiguous, most attempts %d, exhausted %d, clamps %d / %d"
          % (name, n, h, share, d["attempts"].max(), d["exhausted"], d["clamped_bottom"], d["clamped_top"]))
    assert share <= 1e-3
    R.check_replay(CASES[name], d, n)
    c = CASES[name]
    x = d["events"][:, :c.D].astype(np.float64)
    assert np.all((x >= np.asarray(c.lower)) & (x < np.asarray(c.upper))) and np.all(d["events"][:, c.D] == c.dataset)
    assert np.all(R.midpoint_distance(d["xd"]) == d["mid"])
    if d["exhausted"] == 0:
        assert R.compare(d["events"], d, name)["ok"]              # the plain replay changes none against itself


CONTROL = {"one_minus_p": R.tail_control}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_variant_shows(variant):
    """More than 1 % of the events of some case change, and the GPU test's comparison fails there."""
    best = ("", 0.0)
    for name in sorted(CASES):
        if name in ("grid_stride", "exhaustion") and variant != "single_counter":
            continue                                              # (the slow ones, where another case already shows it)
        h, lam, d, _ = replayed(name)
        dv, _ = CASES[name].replay(h, lam, variant=variant)
        share = R.changed_rows(d, dv)
        if share > best[1]:
            best = (name, share)
        if share > 0.01 and d["exhausted"] == 0:
            break
    print("%s over the cases of the GPU test: at most %.3g of the events change (%s)" % (variant, best[1], best[0]))
    if variant in CONTROL:
        assert best[1] < 1e-3                                     # (the module docstring's figures)
        case, h = CONTROL[variant]()
        d, _ = case.replay(h)
        dv, _ = case.replay(h, variant=variant)
        share, name = R.changed_rows(d, dv), case.name
        print("%s on %s: %.3g of the events change" % (variant, name, share))
    assert share > 0.01
    assert d["exhausted"] == 0 and not R.compare(dv["events"], d, "%s on %s" % (variant, name))["ok"]


def test_the_controls_are_what_they_say():
    case, h = R.tail_control()
    d, _ = case.replay(h)
    assert np.mean(R.excused(d)) > 0.9                            # nothing to hold a device to
    # bandwidth_x1e-06: what clamp_before_round hands out beyond `upper` are the draws the sampler moves below it
    h, lam, d, _ = replayed("bandwidth_x1e-06")
    wrong, _ = CASES["bandwidth_x1e-06"].replay(h, lam, variant="clamp_before_round")
    assert np.sum(wrong["events"][:, 0].astype(np.float64) >= 0.2) == d["clamped_top"] > 0.01 * len(d["row"])


def test_a_single_row_no_events_and_cuts_equal_to_the_domain():
    h = np.array([0.4])
    one = R.draw(np.array([[10.5]], np.float32), [7], np.ones(8), h, [0.0], [10.0], 5000, 3)
    assert np.all(one["row"] == 7) and one["exhausted"] == 0
    s = 10.5 * (0.4 / R.KLOG)
    x = one["events"][:, 0].astype(np.float64)
    assert abs(x.mean() - s) < 5 * 0.4 / math.sqrt(5000) and abs(x.std() - 0.4) < 0.03
    none = R.draw(np.array([[10.5]], np.float32), [7], np.ones(8), h, [0.0], [10.0], 0, 3)
    assert none["events"].shape == (0, 2) and none["exhausted"] == 0 and R.compare(none["events"], none)["ok"]
    # cuts equal to the domain (bottom, top as floats): nothing is redrawn, the same events
    c = CASES["D2_seed0"]
    hh, lam, d, _ = replayed("D2_seed0")
    rows_c, idx, fragile = R.prepare(c.table, c.nfields, 2, c.lower, c.upper, hh)
    ends = [R.end_floats(c.lower[k], c.upper[k]) for k in range(2)]
    cut = R.draw(rows_c, idx, lam, hh, c.lower, c.upper, c.nevents, c.seed, [e[0] for e in ends], [e[1] for e in ends],
                 fragile=fragile)
    assert np.all(cut["attempts"] == 1) and cut["events"].tobytes() == d["events"].tobytes()


@pytest.mark.parametrize("lo,hi", [(0.1, 0.2), (0.2, 1.0), (-1.0, 1.0), (0.7, 0.8)])
def test_bottom_and_top(lo, hi):
    """Samples on both ends under a bandwidth of two floats: every event inside the domain, the end floats reached."""
    b, t = R.end_floats(lo, hi)
    assert lo <= float(b) and float(np.nextafter(b, np.float32(-np.inf))) < lo
    assert float(t) < hi <= float(np.nextafter(t, np.float32(np.inf)))
    x = np.array([b, np.nextafter(b, np.float32(np.inf)), t, np.nextafter(t, np.float32(-np.inf))], np.float32)
    h = np.array([2 * float(np.nextafter(t, np.float32(np.inf)) - t)])
    rows_c, idx, fragile = R.prepare(x[:, None], 1, 1, [lo], [hi], h)
    assert len(idx) == 4
    d = R.draw(rows_c, idx, np.ones(4), h, [lo], [hi], 20000, 5, fragile=fragile)
    e = d["events"][:, 0]
    assert np.all(e.astype(np.float64) >= lo) and np.all(e.astype(np.float64) < hi)
    assert np.any(e == b) and np.any(e == t)
    assert d["clamped_top"] > 0                                   # hi is a float or rounds up to one: xd rounds onto it
    assert (d["clamped_bottom"] > 0) == (float(np.float32(lo)) < lo)
