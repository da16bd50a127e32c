"""The histogram event sampler (sxmc_hist_random_sample) restated in numpy with integers and f64, vectorised over
events, and the checks of its law that the CPU and the GPU tests share.

The contract (include/sxmc_hip.h, the comment of random_sample_kernel):

  cdf       inclusive uint32 prefix sum of the flat row-major histogram; total = cdf[-1]
  words     event e, attempt t: Philox4x32-10, counter words (e lo, e hi, t, 0), key (seed lo, seed hi) -> x, y, z, w
  bin       target = (x * total) >> 32; the first bin with cdf > target
  unravel   the last observable fastest
  point     per observable k, with the words y, z, w in this order:
            xd = lower + (idx + (word + 0.5) * 2^-32) * width, width = (upper - lower) / nbins, each operation in f64
  float     xf = (float)xd, then moved one float at a time (at most SETTLE_STEPS) towards the bin while the evaluator's
            look-up of xf -- domain test lower <= xf < upper and (int)((xf - lower) * (nbins / (upper - lower))), in
            f64 on the float -- does not give idx; a bin that holds no float at all: the in-domain float nearest to xd
  cuts      on the float: redrawn (next attempt, bin and point) while xf > hi or xf < lo in any observable; an event
            that has not passed after ATTEMPTS attempts is exhausted, and the call fails

draw() returns the events, the flat bin drawn for each and the attempt counts.  `variant` makes it wrong on purpose, one
way at a time: the negative controls of tests/test_hist_sample_reference_cpu.py."""
import math

import numpy as np

from tests.helpers import philox4x32_10

ATTEMPTS = 1024
SETTLE_STEPS = 4
VARIANTS = ("ge", "first_fastest", "reuse_word", "clamp_cuts", "no_float_step")
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10_np(ctr, key):
    """tests/helpers.philox4x32_10 over arrays: ctr = 4 and key = 2 uint64 arrays (or scalars) holding 32-bit words."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, np.uint64) for k in key)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & U32, p1 & U32, ((p0 >> s32) ^ c3 ^ k1) & U32, p0 & U32
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c0, c1, c2, c3


def words(events, attempts, seed):
    """The four words of (event, attempt) under `seed`: arrays of uint64."""
    e = np.asarray(events, np.uint64)
    t = np.asarray(attempts, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10_np((e & U32, e >> np.uint64(32), t & U32, np.zeros_like(e)),
                            (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))


class Geometry:
    """lower, upper (f64), nbins and what the evaluator derives from them."""

    def __init__(self, lower, upper, nbins):
        self.lower = np.asarray(lower, np.float64).reshape(-1)
        self.upper = np.asarray(upper, np.float64).reshape(-1)
        self.nbins = np.asarray(nbins, np.int64).reshape(-1)
        self.nobs = self.nbins.size
        self.scale = self.nbins / (self.upper - self.lower)         # the look-up's (pdfz.cpp:366-368)
        self.width = (self.upper - self.lower) / self.nbins         # the sampler's
        self.total_nbins = int(np.prod(self.nbins))
        self.stride = np.array([int(np.prod(self.nbins[k + 1:])) for k in range(self.nobs)], np.int64)


def lookup_axis(x, geom, k):
    """SetEvalPoints' arithmetic on one observable, in f64 on the float values: the index, or -1 outside the domain
    (an index that reaches nbins is returned as it is: it is no bin of this axis)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    inside = (x >= geom.lower[k]) & (x < geom.upper[k])
    with np.errstate(invalid="ignore"):
        idx = ((x - geom.lower[k]) * geom.scale[k]).astype(np.int64)
    return np.where(inside, idx, -1)


def lookup(events, geom):
    """The flat bin SetEvalPoints reads for each row of `events` (observables first), -1 outside the domain."""
    flat = np.zeros(events.shape[0], np.int64)
    bad = np.zeros(events.shape[0], bool)
    for k in range(geom.nobs):
        i = lookup_axis(events[:, k], geom, k)
        bad |= (i < 0) | (i >= geom.nbins[k])
        flat += i * geom.stride[k]
    return np.where(bad, -1, flat)


def domain_floats(geom, k):
    """(bottom, top): the smallest float >= lower and the largest float < upper."""
    lo, hi = geom.lower[k], geom.upper[k]
    b, t = np.float32(lo), np.float32(hi)
    if float(b) < lo:
        b = np.nextafter(b, np.float32(np.inf))
    while not float(t) < hi:
        t = np.nextafter(t, np.float32(-np.inf))
    return b, t


def side(xf, idx, geom, k):
    """-1 where the float lies below bin idx of observable k under the look-up, +1 above, 0 inside."""
    x = xf.astype(np.float64)
    j = ((x - geom.lower[k]) * geom.scale[k]).astype(np.int64)
    s = np.where(j < idx, -1, np.where(j > idx, 1, 0))
    s = np.where(x < geom.upper[k], s, 1)
    return np.where(x >= geom.lower[k], s, -1)


def settle(xd, idx, geom, k):
    """The float step.  Returns (xf, nofloat): nofloat marks the draws whose bin holds no float32."""
    xf0 = xd.astype(np.float32)
    xf = xf0.copy()
    for _ in range(SETTLE_STEPS):
        s = side(xf, idx, geom, k)
        if not s.any():
            break
        xf = np.where(s < 0, np.nextafter(xf, np.float32(np.inf)),
                      np.where(s > 0, np.nextafter(xf, np.float32(-np.inf)), xf))
    nofloat = side(xf, idx, geom, k) != 0
    if nofloat.any():
        bottom, top = domain_floats(geom, k)
        near = np.where(xf0.astype(np.float64) >= geom.lower[k], xf0, bottom)
        near = np.where(near.astype(np.float64) < geom.upper[k], near, top)
        xf = np.where(nofloat, near, xf)
    return xf, nofloat


def draw(bins, geom, nevents, seed, lowers=None, uppers=None, dataset=0, variant=None):
    """The sampler.  Returns a dict: events float32 [n, nobs + 1], flat int64 [n] (the bin drawn), attempts int64 [n]
    (how many were made, 1 .. ATTEMPTS), exhausted (how many events passed no attempt; the device call then fails),
    nofloat bool [n] (drawn in a bin that holds no float32 in some observable)."""
    assert variant is None or variant in VARIANTS
    bins = np.asarray(bins, np.uint32).reshape(-1)
    assert bins.size == geom.total_nbins and geom.nobs <= 3
    cdf = np.cumsum(bins.astype(np.uint64)).astype(np.uint32)          # wraps like the device's scan would
    total = np.uint64(cdf[-1])
    assert total > 0
    n, D = int(nevents), geom.nobs
    events = np.zeros((n, D + 1), np.float32)
    events[:, D] = np.float32(dataset)
    flat_out = np.zeros(n, np.int64)
    attempts = np.zeros(n, np.int64)
    nofloat_out = np.zeros(n, bool)
    has_cuts = lowers is not None
    if has_cuts:
        cut_lo, cut_hi = np.asarray(lowers, np.float32), np.asarray(uppers, np.float32)
    active = np.arange(n, dtype=np.int64)
    for t in range(ATTEMPTS):
        if active.size == 0:
            break
        w = words(active, np.full(active.size, t), seed)
        target = ((w[0] * total) >> np.uint64(32)).astype(np.uint32)
        flat = np.searchsorted(cdf, target, side="left" if variant == "ge" else "right").astype(np.int64)
        rest = flat.copy()
        idx = [None] * D
        for k in (range(D) if variant == "first_fastest" else range(D - 1, -1, -1)):
            idx[k] = rest % geom.nbins[k]
            rest = rest // geom.nbins[k]
        ok = np.ones(active.size, bool)
        nofloat = np.zeros(active.size, bool)
        x = np.zeros((active.size, D), np.float32)
        for k in range(D):
            word = w[0] if (variant == "reuse_word" and k == 0) else w[1 + k]
            u = (word.astype(np.float64) + 0.5) * 2.3283064365386963e-10
            xd = geom.lower[k] + (idx[k].astype(np.float64) + u) * geom.width[k]
            if variant == "no_float_step":
                xf = xd.astype(np.float32)
            else:
                xf, nf = settle(xd, idx[k], geom, k)
                nofloat |= nf
            if has_cuts:
                if variant == "clamp_cuts":
                    xf = np.minimum(np.maximum(xf, cut_lo[k]), cut_hi[k])
                else:
                    ok &= ~((xf > cut_hi[k]) | (xf < cut_lo[k]))
            x[:, k] = xf
        # an event keeps what its last attempt drew, as the kernel's registers do
        events[active, :D] = x
        flat_out[active] = flat
        attempts[active] = t + 1
        nofloat_out[active] = nofloat
        active = active[~ok]
    return dict(events=events, flat=flat_out, attempts=attempts, exhausted=int(active.size), nofloat=nofloat_out)


# ------------------------------------------------------------------------------------ the law, without the replica
def wilson_hilferty_sf(chi2, k):
    """tests/test_gpu_kde_sample.wilson_hilferty_sf (that module needs the device library's tests; the same formula)."""
    z = ((chi2 / k) ** (1.0 / 3.0) - (1 - 2.0 / (9 * k))) / math.sqrt(2.0 / (9 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


P_MIN = 1e-4        # the convention of tests/test_gpu_kde_sample.py: p > 1e-4


def chi2_p(counts, expect, sf=wilson_hilferty_sf):
    """Pearson chi-square of counts against expect (same total) over the cells with expectation >= 5.  Returns
    (p, cells used, events in the other cells, expectation of the other cells)."""
    counts, expect = np.asarray(counts, np.float64).ravel(), np.asarray(expect, np.float64).ravel()
    use = expect >= 5
    k = int(use.sum()) - 1
    if k < 1:
        return 1.0, int(use.sum()), float(counts[~use].sum()), float(expect[~use].sum())
    chi2 = float(((counts[use] - expect[use]) ** 2 / expect[use]).sum())
    return sf(chi2, k), int(use.sum()), float(counts[~use].sum()), float(expect[~use].sum())


def kept_fraction(geom, k, lowers, uppers):
    """Per bin of observable k: (a, b) the part of the bin inside the cuts [lo, hi] (f64 of the float cuts), and its
    share of the bin."""
    edges = geom.lower[k] + np.arange(geom.nbins[k] + 1) * geom.width[k]
    a, b = edges[:-1].copy(), edges[1:].copy()
    if lowers is not None:
        a = np.maximum(a, float(np.float32(lowers[k])))
        b = np.minimum(b, float(np.float32(uppers[k])))
    frac = np.clip((b - a) / geom.width[k], 0.0, 1.0)
    return a, b, frac


def law_report(events, rb, bins, geom, lowers=None, uppers=None, sf=wilson_hilferty_sf):
    """Every statistical check of one drawn set, from the events alone (rb: the look-up of the events, e.g. the
    oracle's set_eval_points).  Returns a dict of named booleans (all must hold) and prints the figures.

      bins        chi-square of the looked-up bins against bins / norm -- under cuts against the conditional law, a
                  partially cut bin weighted by its uncut share -- over all bins with expectation >= 5
      rest        the events in the other bins, bounded as test_law_2d_with_all_systematics bounds them
      empty       no event in a bin without content (or entirely outside the cuts)
      inside_k    the position inside the (kept part of the) bin, pooled over bins: 64 sub-cells
      joint       (2-D, 3-D) the positions of all observables together: 8 x 8 (x 8) sub-cells
      perbin_k    the position in 8 sub-cells bin by bin (bins with expectation >= 40): what sees a position that
                  depends on the bin
      unique      (2-D, 3-D) no row is drawn twice"""
    D = geom.nobs
    n = events.shape[0]
    bins = np.asarray(bins, np.float64).reshape(-1)
    out = {}
    weight = bins.copy().reshape(tuple(geom.nbins))
    parts = []
    for k in range(D):
        a, b, frac = kept_fraction(geom, k, lowers, uppers)
        parts.append((a, b))
        shape = [1] * D
        shape[k] = -1
        weight = weight * frac.reshape(shape)
    weight = weight.ravel()
    expect = n * weight / weight.sum()
    out["lookup"] = bool(np.all(rb >= 0))
    counts = np.bincount(rb[rb >= 0], minlength=geom.total_nbins).astype(np.float64)
    p, used, rest, rest_expect = chi2_p(counts, expect, sf)
    print("bins: p = %.3g over %d bins; %d events in the others (expected %.1f)" % (p, used, rest, rest_expect))
    out["bins"] = p > P_MIN
    out["rest"] = rest <= 5 * max(1.0, rest_expect) + 20
    out["empty"] = counts[weight == 0].sum() == 0
    # the position inside the kept part of the bin, in f64 from the float event
    pos = np.zeros((n, D))
    safe = np.maximum(rb, 0)
    for k in range(D):
        idx = (safe // geom.stride[k]) % geom.nbins[k]
        a, b = parts[k]
        span = np.where(b[idx] > a[idx], b[idx] - a[idx], 1.0)
        pos[:, k] = (events[:, k].astype(np.float64) - a[idx]) / span
    for k in range(D):
        cell = np.clip(np.floor(pos[:, k] * 64), 0, 63).astype(np.int64)
        p, _, _, _ = chi2_p(np.bincount(cell, minlength=64), np.full(64, n / 64.0), sf)
        print("inside bins, observable %d: p = %.3g" % (k, p))
        out["inside_%d" % k] = p > P_MIN
        sub = np.clip(np.floor(pos[:, k] * 8), 0, 7).astype(np.int64)
        table = np.bincount(safe * 8 + sub, minlength=geom.total_nbins * 8).reshape(-1, 8).astype(np.float64)
        rows = expect >= 40
        if rows.sum() * 7 >= 1:
            e = np.repeat(table[rows].sum(axis=1, keepdims=True) / 8.0, 8, axis=1)
            chi2 = float((((table[rows] - e) ** 2) / np.maximum(e, 1e-300)).sum())
            p = sf(chi2, int(rows.sum()) * 7)
            print("inside each of %d bins, observable %d: p = %.3g" % (rows.sum(), k, p))
            out["perbin_%d" % k] = p > P_MIN
    if D > 1:
        cell = np.zeros(n, np.int64)
        for k in range(D):
            cell = cell * 8 + np.clip(np.floor(pos[:, k] * 8), 0, 7).astype(np.int64)
        p, _, _, _ = chi2_p(np.bincount(cell, minlength=8 ** D), np.full(8 ** D, n / float(8 ** D)), sf)
        print("inside bins, jointly: p = %.3g" % p)
        out["joint"] = p > P_MIN
        # (one observable alone has too few floats per bin for 1e5 and more events never to meet)
        rows = np.ascontiguousarray(events[:, :D]).view([("", np.float32)] * D).ravel()
        out["unique"] = np.unique(rows).size == n
    return out


def rows_in_common(a, b, D):
    """How many rows (observables only) two event sets share."""
    va = np.ascontiguousarray(a[:, :D]).view([("", np.float32)] * D).ravel()
    vb = np.ascontiguousarray(b[:, :D]).view([("", np.float32)] * D).ravel()
    return int(np.intersect1d(va, vb).size)


# ------------------------------------------------------------------------------------ the cases both test files run
class Case:
    """A histogram as the tests fill it: a sample table, systematics and their parameters over a geometry."""

    def __init__(self, name, lower, upper, nbins, table, systs, params, dataset=0):
        self.name, self.geom = name, Geometry(lower, upper, nbins)
        self.table = np.ascontiguousarray(table, np.float32)
        self.nfields = self.table.shape[1]
        self.systs, self.params, self.dataset = systs, list(params), dataset

    def oracle_bins(self):
        """The histogram by the CPU oracle (what the device fill equals bit for bit: tests/test_gpu_pdfz.py)."""
        from oracle import oracle
        g = oracle.HistGeometry(self.geom.lower, self.geom.upper, [int(b) for b in self.geom.nbins])
        bins, _ = oracle.bin_samples(g, self.table, self.nfields, self.systs, np.asarray(self.params, np.float64))
        return bins


C3_SYSTS = [dict(type="shift", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
            dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])]
C3_PARAMS = [0.02, -0.004, 0.03]
SEEDS = (0, 1, 2 ** 63 - 1, 0x0123456789ABCDEF)
COUNTS = (1, 255, 256, 257)
BIG_COUNT = 2 ** 20 + 3                      # above 4096 x 256: the grid-stride loop runs


def case_1d(n=60000):
    rng = np.random.default_rng(101)
    t = 10 * rng.random(n) * rng.random(n)
    tab = np.stack([t + rng.normal(0, 0.3, n), t, np.zeros(n)], axis=1)
    return Case("1d", [0.0], [10.0], [20], tab, [dict(type="scale", obs=0, pars=[0]),
                                                 dict(type="resolution_scale", obs=0, true_obs=1, pars=[1])],
                [0.01, 0.05])


def case_2d(n=80000):
    rng = np.random.default_rng(102)
    t = rng.normal(4.0, 2.0, n)
    r = 6.0 * rng.random(n) ** (1.0 / 3.0)
    tab = np.stack([t + rng.normal(0, 0.3, n), r, t, np.zeros(n)], axis=1)
    return Case("2d", [0.0, 0.0], [10.0, 6.0], [25, 12], tab,
                [dict(type="shift", obs=1, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=2, pars=[1])],
                [-0.03, 0.04])


def case_3d(n=300000, seed=103):
    """The shape of BASELINE config 3 (fields e, r, c, e_true, dataset), which the ordered and boxed forms apply to."""
    rng = np.random.default_rng(seed)
    e_true = rng.normal(2.5, 1.2, n)
    tab = np.stack([e_true + rng.normal(0, 0.3, n), 6.0 * rng.random(n) ** (1.0 / 3.0), rng.uniform(-1, 1, n), e_true,
                    np.zeros(n)], axis=1)
    return Case("3d", [0.0, 0.0, -1.0], [10.0, 6.0, 1.0], [20, 20, 20], tab, C3_SYSTS, C3_PARAMS)


SHAPE_GEOM = ([0.0, 0.0, -1.0], [6.0, 5.0, 1.0], [6, 5, 4])
SHAPE_SYSTS = [dict(type="shift", obs=0, pars=[0])]


def _centres(geom, flat, rng, n):
    """n samples inside the bins `flat` (middle halves, so that the small shift keeps them there)."""
    flat = np.asarray(flat)
    pick = flat[rng.integers(0, flat.size, n)]
    cols = []
    for k in range(geom.nobs):
        idx = (pick // geom.stride[k]) % geom.nbins[k]
        cols.append(geom.lower[k] + (idx + 0.25 + 0.5 * rng.random(n)) * geom.width[k])
    return np.stack(cols + [np.zeros(n)], axis=1)


def shape_cases():
    """Dense, mostly empty, one non-empty bin (first, last, middle), the last bin of every axis in 1, 2 and 3
    observables, and neighbouring counts that differ by 1e5."""
    g3 = Geometry(*SHAPE_GEOM)
    rng = np.random.default_rng(104)
    out = []
    every = np.arange(g3.total_nbins)
    out.append(Case("dense", *SHAPE_GEOM, _centres(g3, every, rng, 50000), SHAPE_SYSTS, [0.01]))
    out.append(Case("mostly_empty", *SHAPE_GEOM, _centres(g3, rng.choice(every, 14, replace=False), rng, 40),
                    SHAPE_SYSTS, [0.01]))
    for name, flat in (("one_first", 0), ("one_last", g3.total_nbins - 1), ("one_middle", 67)):
        out.append(Case(name, *SHAPE_GEOM, _centres(g3, [flat], rng, 500), SHAPE_SYSTS, [0.01]))
    for D in (1, 2):
        g = Geometry(SHAPE_GEOM[0][:D], SHAPE_GEOM[1][:D], SHAPE_GEOM[2][:D])
        out.append(Case("last_of_every_axis_%dd" % D, g.lower, g.upper, g.nbins,
                        _centres(g, [g.total_nbins - 1], rng, 300), SHAPE_SYSTS, [0.01]))
    g1 = Geometry([0.0], [8.0], [8])
    steps = np.concatenate([np.repeat(np.arange(0, 8, 2), 1), np.repeat(np.arange(1, 8, 2), 100001)])
    tab = np.stack([steps + 0.25 + 0.5 * rng.random(steps.size), np.zeros(steps.size)], axis=1)
    out.append(Case("steps_of_1e5", g1.lower, g1.upper, g1.nbins, tab, SHAPE_SYSTS, [0.01]))
    return out


FAR = {"1000": (1000.0, 1001.0, 1000), "3e4": (30000.0, 30010.0, 20), "1e6": (1e6, 1e6 + 10, 20),
       "-2.5e5": (-250000.0, -249990.0, 20)}
FAR_EVENTS = 1000000
FAR_SEED = 20261


def far_case(name, n=200000):
    """A domain far from zero, filled uniformly; a shift of a quarter bin."""
    lo, hi, nb = FAR[name]
    rng = np.random.default_rng(105)
    x = lo + (hi - lo) * rng.random(n)
    tab = np.stack([x, x, np.zeros(n)], axis=1)
    return Case("far_" + name, [lo], [hi], [nb], tab, [dict(type="shift", obs=0, pars=[0])], [0.25 * (hi - lo) / nb])


# (name, lowers, uppers, events, seed) over case_3d(): decided with the replica on the CPU
CUTS_3D = {
    "through_bins": ([1.1, 2.03, -0.55], [4.2, 5.01, 0.52], 200000, 7),
    "one_in_sixty": ([2.0, 3.0, -0.5], [3.0, 4.0, 0.1], 50000, 8),
    "one_in_500": ([2.0, 3.0, -0.5], [2.5, 3.5, -0.17], 8, 9),
    "one_in_500_fails": ([2.0, 3.0, -0.5], [2.5, 3.5, -0.17], 2000, 10),
}
CUTS_1D = {"through_bins": ([2.2], [6.9], 100000, 16), "one_bin": ([3.0], [3.4999], 20000, 18)}
CUTS_2D = {"one_bin": ([4.0, 5.5], [4.3999, 5.9999], 5000, 19)}

# name -> (case, events, seed, cuts): the statistical assertions of tests/test_gpu_hist_sample.py, each decided on the
# CPU by tests/test_hist_sample_reference_cpu.py with the same seed (the device stream equals the replica's)
LAW_CASES = {
    "1d": (case_1d, 200000, 11, None),
    "2d": (case_2d, 400000, 12, None),
    "3d": (case_3d, 400000, 13, None),
    "3d_other_seed": (case_3d, 400000, 17, None),
    "1d_cuts": (case_1d, 100000, 16, CUTS_1D["through_bins"][:2]),
    "3d_cuts": (case_3d, 200000, 7, CUTS_3D["through_bins"][:2]),
}

