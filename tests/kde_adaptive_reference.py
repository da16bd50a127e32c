"""The contract of pdfz::EvalKernel with adaptive (sample-point) bandwidths (sxmc_amd/include/sxmc/pdfz.h, class
EvalKernel, "Adaptive"; include/sxmc_hip.h, sxmc_kde_create_adaptive) restated in numpy f64, on top of
tests/kde_reference.py: the local factors, the values with the error bound of the adaptive pair kernel's f32 arithmetic,
and the component CDFs of the sampler and the projection.  No device needed.

The factors.  S0 = the n untransformed in-domain samples, h the Scott bandwidths; for every table row i
  f_i = (1/n) sum_{j in S0} w_j prod_d phi((x_id - x_jd) / h_d) / h_d,   w_j = 1 / truncation mass of j at h,
  g = exp(mean_{i in S0} ln f_i),   lambda_i = min(10, max(0.1, (f_i / g)^-alpha)),  10 where f_i is not finite and > 0.

The values.  pdf(x) = (1/norm) sum_{i in domain} w_i prod_d phi((x_d - s_id) / (h_d lambda_i)) / (h_d lambda_i), w_i the
truncation weight at h lambda_i.  In the kernels' units -- c = (x - lower) sqrt(log2(e) / 2) / h with the GLOBAL h,
a_d = c_pd - c_id, q = sum_d a_d^2 -- a term is t = W exp2(-q'), q' = g q, g = 1 / lambda^2, W = w / lambda^D, and the
prefactor 1 / ((2 pi)^(D/2) prod h) is the fixed-bandwidth one.

The bound, derived as kde_reference.py derives its own (u = 2^-24, first order).  The adaptive pair kernel
(kde_pairs_kernel<D, true>) forms q exactly as the fixed one does, so |dq| <= 4 u c_max sum_d |a_d| + (D + 3) u q;
then it multiplies by g, itself rounded to f32: two more roundings, each u relative on q', so
  |dq'| <= g (4 u c_max sum_d |a_d| + (D + 3) u q) + 2 u q' = 4 u c_max g sum_d |a_d| + (D + 5) u q',
and the term moves by ln 2 |dq'| relative.  exp2 is v_exp_f32 (2 u) and W an f32 (u): 3 u as before.  The tile sum in
f32 and the tiles in f64 are unchanged: u sum_i (256 - pos_i) t_i.  Pairs whose exp2 underflows (q' > 126) or whose sums
go subnormal add at most (sum_i W_i) 2^-126.  With S0 = sum t, S1 = sum t g sum_d |a_d|, S2 = sum t q', ST =
sum (256 - pos) t:
  bound = prefactor / norm * (u (ln 2 (4 c_max S1 + (D + 5) S2) + 3 S0 + ST) + 2^-126 sum W) + u |v| + 2^-149.
Against the fixed-bandwidth bound the coordinate term carries g <= 100 (the clip lambda >= 0.1) where narrow kernels
reach the point: the clips are what keeps it finite.  lambda itself is compared at 1e-11 (tests/test_gpu_kde_adaptive.py),
five orders below u, so the values may be compared with this module's own factors.

Planted errors (ADAPTIVE_PLANTS, besides kde_reference.PLANTS), each of which must make the comparison fail:
"fixed" lambda = 1; "sensitivity" alpha * 1.01; "weight" the masses taken at h instead of h lambda; "power" the
lambda^-D factor dropped; "unclipped" no clips (only where factors clip)."""
import math

import numpy as np

from tests.kde_reference import (CSCALE, PLANTS, TILE, U, KdeRef, PAIRS_PER_CHUNK, _erfc, phi, ref_bandwidths,
                                 ref_transform, truncation_mass)

ADAPTIVE_PLANTS = ("fixed", "sensitivity", "weight", "power")   # and "unclipped" on a table whose factors clip
LAMBDA_MIN, LAMBDA_MAX = 0.1, 10.0


# ------------------------------------------------------------------ the factors
def ref_pilot(samples, nfields, nobs, lower, upper, scale):
    """(f [rows], inside [rows] bool, h): the fixed-bandwidth PDF at zero systematics at every table row."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.all((x >= lower) & (x < upper), axis=1)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)
    s0 = x[inside]
    n = len(s0)
    w = 1.0 / truncation_mass(s0, h, lower, upper)
    f = np.empty(len(x))
    step = max(1, PAIRS_PER_CHUNK // max(n * nobs, 1))
    c = 1.0 / ((2 * math.pi) ** (nobs / 2) * np.prod(h))
    with np.errstate(invalid="ignore"):
        for a in range(0, len(x), step):
            z = (x[a:a + step, None, :] - s0[None, :, :]) / h        # the difference first, then the bandwidth
            f[a:a + step] = np.exp(-0.5 * (z * z).sum(axis=2)) @ w
    return f * c / n, inside, h


def ref_local_factors(samples, nfields, nobs, lower, upper, scale, alpha, clip=True):
    """lambda of every table row (f64 [rows])."""
    f, inside, _ = ref_pilot(samples, nfields, nobs, lower, upper, scale)
    g = math.exp(float(np.sum(np.log(f[inside]))) / int(inside.sum()))
    good = np.isfinite(f) & (f > 0)
    lam = np.full(len(f), LAMBDA_MAX)
    with np.errstate(over="ignore"):
        lam[good] = (f[good] / g) ** (-alpha)
    if clip:
        lam[good] = np.minimum(LAMBDA_MAX, np.maximum(LAMBDA_MIN, lam[good]))
    return lam


def mass_at(s, hw, lower, upper):
    """prod_d [Phi((upper_d - s_d)/hw_d) - Phi((lower_d - s_d)/hw_d)] with a bandwidth per sample and observable."""
    r2 = 1.0 / (hw * math.sqrt(2.0))
    return np.prod(0.5 * (_erfc((s - upper) * r2) - _erfc((s - lower) * r2)), axis=1)


# ------------------------------------------------------------------ the values
def ref_kde_adaptive(samples, nfields, nobs, lower, upper, scale, alpha, systs, params, points, dataset=0, plant=None):
    """The adaptive contract in f64 with the kernels' bound (module docstring); `plant` one of ADAPTIVE_PLANTS,
    "unclipped" or kde_reference.PLANTS gives a reference with that one error."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)
    if plant == "fixed":
        lam = np.ones(np.asarray(samples).size // nfields)
    else:
        lam = ref_local_factors(samples, nfields, nobs, lower, upper, scale,
                                alpha * 1.01 if plant == "sensitivity" else alpha, clip=plant != "unclipped")
    if plant == "bandwidth":
        h = h * (1 + 1e-3)
    s = ref_transform(samples, nfields, systs, params)[:, :nobs]
    with np.errstate(invalid="ignore"):
        inside = np.all((s >= lower) & (s < upper), axis=1)
    pos = np.flatnonzero(inside) % TILE
    s, lam = s[inside], lam[inside]
    norm = int(inside.sum()) + (1 if plant == "norm" else 0)
    if plant == "untruncated":
        w = np.ones(len(s))
    elif plant == "weight":
        w = 1.0 / truncation_mass(s, h, lower, upper)
    else:
        w = 1.0 / mass_at(s, h[None, :] * lam[:, None], lower, upper)
    W = w if plant == "power" else w / lam ** nobs
    g = 1.0 / (lam * lam)
    if plant == "swap":
        s = s[:, [1, 0] + list(range(2, nobs))]
    pts = np.asarray(points, np.float32).reshape(-1, nobs + 1)
    x = pts[:, :nobs].astype(np.float64)
    with np.errstate(invalid="ignore"):
        in_dom = np.all((x >= lower) & (x < upper), axis=1)
    mine = in_dom & (pts[:, nobs] == np.float32(dataset))
    cs = CSCALE / h
    cx, cq = (x - lower) * cs, (s - lower) * cs
    c_max = float(max(np.abs(cq).max(initial=0.0), np.abs(cx[mine]).max(initial=0.0)))
    S = np.zeros((4, len(x)))
    Wt = W * (TILE - pos)
    step = max(1, PAIRS_PER_CHUNK // max(len(s) * nobs, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(x), step):
            b = min(len(x), a + step)
            A = cx[a:b, None, :] - cq[None, :, :]
            q = (A * A).sum(axis=2) * g[None, :]
            e = np.exp2(-q)
            S[0, a:b] = e @ W
            S[1, a:b] = (e * np.abs(A).sum(axis=2)) @ (W * g)
            S[2, a:b] = (e * q) @ W
            S[3, a:b] = e @ Wt
    c = 1.0 / ((2 * math.pi) ** (nobs / 2) * np.prod(h))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = S[0] * c / norm if norm else np.full(len(x), np.nan)
        bound = (c / norm if norm else 0.0) * (U * (math.log(2) * (4 * c_max * S[1] + (nobs + 5) * S[2]) + 3 * S[0]
                                                    + S[3]) + 2.0 ** -126 * W.sum())
    bound = bound + U * np.abs(np.nan_to_num(out)) + 2.0 ** -149
    out[in_dom & ~mine] = 0.0
    out[~in_dom] = np.nan
    return KdeRef(out, norm, h, bound, c_max)


def moved_with_factors(samples, nfields, nobs, lower, upper, scale, alpha, systs, params):
    """(s [n, D], lambda [n]): the moved in-domain samples in table order and the factors of their table rows."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    lam = ref_local_factors(samples, nfields, nobs, lower, upper, scale, alpha)
    s = ref_transform(samples, nfields, systs, params)[:, :nobs]
    with np.errstate(invalid="ignore"):
        inside = np.all((s >= lower) & (s < upper), axis=1)
    return s[inside], lam[inside]


# ------------------------------------------------------------------ the sampler's law
def adaptive_component_cdf(x, s, hw, lo, hi):
    """[len(x), len(s)]: the CDF at every x of every component, N(s_i, hw_i^2) truncated to [lo, hi) (one observable;
    hw = h lambda, one per component)."""
    pa, pb = phi((lo - s) / hw), phi((hi - s) / hw)
    return (phi((np.asarray(x)[:, None] - s[None, :]) / hw[None, :]) - pa[None, :]) / (pb - pa)[None, :]


def adaptive_mixture_cdf(x, s, hw, lo, hi, chunk=512):
    out = np.empty(len(x))
    for a in range(0, len(x), chunk):
        out[a:a + chunk] = adaptive_component_cdf(x[a:a + chunk], s, hw, lo, hi).mean(axis=1)
    return out


def adaptive_ks_distance(events, s, hw, lo, hi):
    """sup |F_N - F| against the adaptive mixture CDF (a fine grid, linearly interpolated)."""
    grid = np.linspace(lo, hi, 4001)
    F = np.interp(np.sort(events), grid, adaptive_mixture_cdf(grid, s, hw, lo, hi))
    n = len(events)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)))


# ------------------------------------------------------------------ the projection
def adaptive_marginal_from_u(u, lam, lower, upper, h, nbins):
    """(shares [nbins], masses [n]): per sample and bin [Phi((t_j+1 - u)/lambda) - Phi((t_j - u)/lambda)] over
    [Phi((T - u)/lambda) - Phi(-u/lambda)], u = (s - lower) / h, t_j the edges of tests/project_reference.py."""
    from tests.project_reference import bin_edges_t
    u, lam = np.asarray(u, np.float64), np.asarray(lam, np.float64)
    if u.size == 0:
        return np.zeros(nbins), np.zeros(0)
    t = bin_edges_t(lower, upper, h, nbins)
    mass = phi((t[-1] - u) / lam) - phi(-u / lam)
    cdf = phi((t[:, None] - u[None, :]) / lam[None, :])
    share = ((cdf[1:] - cdf[:-1]) / mass[None, :]).sum(axis=1) / u.size
    return share, mass


def ref_adaptive_marginal(samples, nfields, nobs, lower, upper, scale, alpha, systs, params, obs, nbins, rounded=True,
                          factor_scale=1.0):
    """(shares, u_max, mass_min, lambda_min) of sxmc_kde_project on an adaptive evaluator.  rounded: u through the
    prepass's f32 scaled coordinate, as the device reads it; else from the unrounded f64 samples.  factor_scale != 1: a
    reference with a planted error (every lambda off by that factor)."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)[obs]
    s, lam = moved_with_factors(samples, nfields, nobs, lower, upper, scale, alpha, systs, params)
    s = s[:, obs]
    if rounded:
        u = ((s - lower[obs]) * (CSCALE / h)).astype(np.float32).astype(np.float64) / CSCALE
    else:
        u = (s - lower[obs]) / h
    share, mass = adaptive_marginal_from_u(u, lam * factor_scale, lower[obs], upper[obs], h, nbins)
    return share, float(np.abs(u).max(initial=0.0)), float(mass.min(initial=1.0)), float(lam.min(initial=1.0))


__all__ = ["ADAPTIVE_PLANTS", "PLANTS", "ref_pilot", "ref_local_factors", "ref_kde_adaptive", "moved_with_factors",
           "adaptive_component_cdf", "adaptive_mixture_cdf", "adaptive_ks_distance", "adaptive_marginal_from_u",
           "ref_adaptive_marginal"]
