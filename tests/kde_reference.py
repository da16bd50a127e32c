"""The contract of pdfz::EvalKernel (sxmc_amd/include/sxmc/pdfz.h, class EvalKernel) restated in numpy f64, and the
error bound of the kernels' f32 arithmetic (sxmc_amd/csrc/kde_kernels.hip): the reference every kernel-density test
compares with.  No device needed.

The bound.  With u = 2^-24, c = (x - lower) sqrt(log2(e) / 2) / h a scaled coordinate (c_max the largest over the
compared points and the in-domain samples) and, per pair, a_d = c_pd - c_id, q = sum_d a_d^2 and the term
t = w exp2(-q) (= w exp(-z^2 / 2)), the kernels
  - round each c to f32 (|dc| <= u c_max) and subtract in f32 (<= u |a_d|): |dq| <= 4 u c_max sum_d |a_d| + (D + 3) u q
    to first order, with the squares and fused adds, so the term moves by ln 2 |dq| relative;
  - take exp2 with v_exp_f32 (1 ulp: 2 u) and the weight as f32 (u);
  - add the terms of a 256-row tile in f32: the running sum after row j rounds once, so the tile errs by at most
    u sum_j acc_j = u sum_i (256 - (row_i mod 256)) t_i (rows in table order);
  - add the tiles in f64 and round the value to f32 (u |v|).
Pairs whose exp2 underflows (q > 126) or whose sums go subnormal add at most (sum_i w_i) 2^-126 to the sum: the
absolute floor.  So, per point, with S0 = sum t, S1 = sum t sum_d |a_d|, S2 = sum t q, ST = sum (256 - pos) t:
  bound = prefactor / norm * (u (ln 2 (4 c_max S1 + (D + 3) S2) + 3 S0 + ST) + 2^-126 sum w) + u |v| + 2^-149.
In relative terms about u (128 + 2.8 c_max A) with A the term-weighted mean of sum_d |a_d|: near 1e-5 for c_max ~ 20,
4e-5 at 200 and growing linearly beyond."""
import math
from dataclasses import dataclass

import numpy as np

try:
    from scipy.special import erfc as _erfc
except ImportError:   # (plain libm, one value at a time)
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

U = 2.0 ** -24
CSCALE = math.sqrt(math.log2(math.e) / 2.0)   # the kernels' sqrt(log2(e) / 2): exp(-z^2 / 2) = exp2(-(z * CSCALE)^2)
TILE = 256                                      # SXMC_KDE_TILE: sample rows per f32 partial sum
PAIRS_PER_CHUNK = 2 ** 22

# the planted errors of the negative controls: each must make the value comparison fail
PLANTS = ("bandwidth", "untruncated", "swap", "norm")


# ------------------------------------------------------------------ the contract (f64)
def ref_transform(samples, nfields, systs, params):
    """Every systematic on every sample, in order (apply_systematic, pdfz.cpp:306-331); p = sum_i c_i x^i."""
    f = np.asarray(samples, np.float32).reshape(-1, nfields).astype(np.float64)
    for s in systs:
        k = s["obs"]
        x = f[:, k]
        p = np.zeros_like(x)
        for i, q in enumerate(s["pars"]):
            p = p + params[q] * (x ** i)
        if s["type"] == "shift":
            f[:, k] = x + p
        elif s["type"] == "scale":
            f[:, k] = x * (1 + p)
        elif s["type"] == "ctscale":
            f[:, k] = 1 + (x - 1) * (1 + p)
        else:
            f[:, k] = x + p * (x - f[:, s["true_obs"]])
    return f


def ref_bandwidths(samples, nfields, nobs, lower, upper, scale):
    """Scott's rule over the untransformed in-domain samples: scale * sigma (n - 1) * n^(-1/(D+4))."""
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    inside = np.all((x >= lower) & (x < upper), axis=1)
    n = int(inside.sum())
    return np.asarray(scale) * x[inside].std(axis=0, ddof=1) * n ** (-1.0 / (nobs + 4))


def truncation_mass(s, h, lower, upper):
    """prod_d [Phi((upper_d - s_d)/h_d) - Phi((lower_d - s_d)/h_d)], written as the kernel writes it (two erfc)."""
    h = np.asarray(h, np.float64)
    s = np.asarray(s, np.float64).reshape(-1, h.size)
    r2 = 1.0 / (h * math.sqrt(2.0))
    return np.prod(0.5 * (_erfc((s - upper) * r2) - _erfc((s - lower) * r2)), axis=1)


def phi(z):
    return 0.5 * _erfc(-np.asarray(z, np.float64) / math.sqrt(2.0))


def component_cdf(x, s, h, lo, hi):
    """[len(x), len(s)]: the truncated Gaussian CDF of every component at every x (one observable)."""
    pa, pb = phi((lo - s) / h), phi((hi - s) / h)
    return (phi((np.asarray(x)[:, None] - s[None, :]) / h) - pa[None, :]) / (pb - pa)[None, :]


def mixture_cdf(x, s, h, lo, hi, chunk=512):
    out = np.empty(len(x))
    for a in range(0, len(x), chunk):
        out[a:a + chunk] = component_cdf(x[a:a + chunk], s, h, lo, hi).mean(axis=1)
    return out


def moved_in_domain(samples, nfields, nobs, lower, upper, systs, params):
    s = ref_transform(samples, nfields, systs, params)[:, :nobs]
    return s[np.all((s >= np.asarray(lower)) & (s < np.asarray(upper)), axis=1)]


@dataclass
class KdeRef:
    values: np.ndarray   # f64 pdf per point (NaN, 0 where the point codes say)
    norm: int
    h: np.ndarray
    bound: np.ndarray    # per point: the kernels' error bound (module docstring)
    c_max: float


def ref_kde(samples, nfields, nobs, lower, upper, scale, systs, params, points, dataset=0, plant=None):
    """The contract in f64, chunked; `plant` one of PLANTS gives a reference with that one error."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)
    if plant == "bandwidth":
        h = h * (1 + 1e-3)
    s = ref_transform(samples, nfields, systs, params)[:, :nobs]
    inside = np.all((s >= lower) & (s < upper), axis=1)
    pos = np.flatnonzero(inside) % TILE                  # the row's place in its tile (rows in table order)
    s = s[inside]
    norm = int(inside.sum()) + (1 if plant == "norm" else 0)
    w = np.ones(len(s)) if plant == "untruncated" else 1.0 / truncation_mass(s, h, lower, upper)
    if plant == "swap":
        s = s[:, [1, 0] + list(range(2, nobs))]
    pts = np.asarray(points, np.float32).reshape(-1, nobs + 1)
    x = pts[:, :nobs].astype(np.float64)
    in_dom = np.all((x >= lower) & (x < upper), axis=1)
    mine = in_dom & (pts[:, nobs] == np.float32(dataset))
    cs = CSCALE / h
    cx, cq = (x - lower) * cs, (s - lower) * cs
    c_max = float(max(np.abs(cq).max(initial=0.0), np.abs(cx[mine]).max(initial=0.0)))
    S = np.zeros((4, len(x)))
    wt = w * (TILE - pos)
    step = max(1, PAIRS_PER_CHUNK // max(len(s) * nobs, 1))
    with np.errstate(invalid="ignore"):                 # (points at infinity: NaN in the sums, NaN values below)
        for a in range(0, len(x), step):
            b = min(len(x), a + step)
            A = cx[a:b, None, :] - cq[None, :, :]
            q = (A * A).sum(axis=2)
            e = np.exp2(-q)
            S[0, a:b] = e @ w
            S[1, a:b] = (e * np.abs(A).sum(axis=2)) @ w
            S[2, a:b] = (e * q) @ w
            S[3, a:b] = e @ wt
    c = 1.0 / ((2 * math.pi) ** (nobs / 2) * np.prod(h))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = S[0] * c / norm if norm else np.full(len(x), np.nan)
        bound = (c / norm if norm else 0.0) * (U * (math.log(2) * (4 * c_max * S[1] + (nobs + 3) * S[2]) + 3 * S[0]
                                                    + S[3]) + 2.0 ** -126 * w.sum())
    bound = bound + U * np.abs(np.nan_to_num(out)) + 2.0 ** -149
    out[in_dom & ~mine] = 0.0
    out[~in_dom] = np.nan
    return KdeRef(out, norm, h, bound, c_max)


# ------------------------------------------------------------------ the comparison
def compare(got, ref):
    """(ok, worst error / bound, worst relative error) of values against a reference: NaN where it has NaN, and
    |got - ref| <= bound everywhere else.  The relative error is reported over the values above 1e-3 of the largest
    (below that the absolute floor rules)."""
    got, want = np.asarray(got, np.float64), np.asarray(ref.values, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False, math.inf, math.inf
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    ratio = float(np.max(err / ref.bound[ok])) if err.size else 0.0
    big = np.abs(want[ok]) >= 1e-3 * np.max(np.abs(want[ok]), initial=0.0)
    rel = float(np.max(err[big] / np.abs(want[ok][big]), initial=0.0))
    return ratio <= 1.0, ratio, rel


def check_values(got, ref, label):
    ok, ratio, rel = compare(got, ref)
    print("%s: c_max %.4g, worst error / bound %.3g, worst relative error %.3g" % (label, ref.c_max, ratio, rel))
    assert ok, "%s: error %.3g x the bound" % (label, ratio)
    return ratio


def check_power(got, reference, plants=PLANTS, label=""):
    """Negative controls: `got` compared with a reference that has one planted error fails, for every plant.
    reference: plant -> KdeRef."""
    for p in plants:
        ok, ratio, _ = compare(got, reference(p))
        print("%s control %s: error %.3g x the bound" % (label, p, ratio))
        assert not ok, "%s: the comparison misses a planted %s error" % (label, p)


# ------------------------------------------------------------------ the kernels' arithmetic, emulated in numpy f32
def emulate_kernel(samples, nfields, nobs, lower, upper, scale, systs, params, points, dataset=0):
    """kde_prepass + kde_pairs + kde_combine in the kernels' precision (f32 coordinates, differences, exp2 and tile sums
    in table order; f64 across tiles): what a correct kernel may compute.  Points of another data set or outside the
    domain as the contract says."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)
    f = ref_transform(samples, nfields, systs, params)[:, :nobs]
    inside = np.all((f >= lower) & (f < upper), axis=1)
    norm = int(inside.sum())
    n = len(f)
    npad = max(TILE, -(-n // TILE) * TILE)
    cs = CSCALE / h
    rows = np.zeros((npad, nobs + 1), np.float32)
    rows[:n][inside, :nobs] = ((f[inside] - lower) * cs).astype(np.float32)
    rows[:n][inside, nobs] = (1.0 / truncation_mass(f[inside], h, lower, upper)).astype(np.float32)
    pts = np.asarray(points, np.float32).reshape(-1, nobs + 1)
    x = pts[:, :nobs].astype(np.float64)
    cx = ((x - lower) * cs).astype(np.float32)
    total = np.zeros(len(x))
    step = max(1, PAIRS_PER_CHUNK // (npad * nobs))
    for a in range(0, len(x), step):
        d = cx[a:a + step, None, :] - rows[None, :, :nobs]
        q = (d * d).sum(axis=2, dtype=np.float32)
        t = (rows[None, :, nobs] * np.exp2(-q)).reshape(len(d), -1, TILE)
        total[a:a + step] = np.cumsum(t, axis=2, dtype=np.float32)[:, :, -1].astype(np.float64).sum(axis=1)
    c = 1.0 / ((2 * math.pi) ** (nobs / 2) * np.prod(h))
    out = (total * c / norm).astype(np.float32).astype(np.float64) if norm else np.full(len(x), np.nan)
    in_dom = np.all((x >= lower) & (x < upper), axis=1)
    out[in_dom & (pts[:, nobs] != np.float32(dataset))] = 0.0
    out[~in_dom] = np.nan
    return out, norm
