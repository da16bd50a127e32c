"""The contract of pdfz::EvalKernel's bandwidth cross-validation (include/sxmc_hip.h, sxmc_kde_cv_scores /
sxmc_kde_cv_select; sxmc_amd/csrc/kde_cv.h) restated in numpy f64: the rows scored, the scores with an error bound, the
grid, the split rule, the choice and the search.  No device needed.

The score.  x the m scored rows (the untransformed in-domain rows, or every ceil(n / max_rows)-th of them, as f64 values
of the floats), h a candidate bandwidth vector, [L_d, U_d) the domain, Phi through erfc:
  M_jd(h)  = Phi((U_d - x_jd)/h_d) - Phi((L_d - x_jd)/h_d) = (erfc((x_jd - U_d) r_d) - erfc((x_jd - L_d) r_d)) / 2,
             r_d = 1 / (h_d sqrt 2)
  f_-i(h)  = 1/(m-1) sum_{j != i} prod_d phi((x_id - x_jd)/h_d) / (h_d M_jd(h))
  score(h) = (1/m) sum_i ln f_-i(h);  the pair j == i is left out (not subtracted), f_-i = 0 gives -inf.

The bound on |d score| of the device's arithmetic (kde_cv_weights / kde_cv_pairs / kde_cv_combine of kde_kernels.hip),
first order in e = 2^-53, the unit roundoff of f64.  A term is t_ij = w_j exp(-q_ij), q_ij = sum_d (x_id - x_jd)^2 g_d,
g_d = 1 / (2 h_d^2), w_j = 1 / (prod_d h_d  prod_d M_jd).
  q      the difference of two f64 values (e), its square (e), g_d (h h: e, the reciprocal: e -- times 2 is exact), the
         product (e) and the multiply-adds over d (at most D - 1 more): |dq| <= (D + 4) e q; exp(-q) moves by |dq|
         relative, and exp itself by 2 e (one ulp of the device's exp): (D + 4) e q + 2 e.
  w_j    each erfc is within E e of its value relative (E = 16: eight ulps, twice what math libraries state for
         their f64 erfc at the worst) and its argument (the difference e, r_d 3 e, the product e) moves it by at most
         5 e |a erfc'(a)| <= 5 e * 0.49; so M_jd, half a difference of an erfc in [1, 2] and one in [0, 1], is within
         e (E (ea + eb) + 5 + |ea - eb|) / |ea - eb| relative.  prod_d h_d (D e), the products over d and with it
         (D e), the reciprocal (e): rho_j = sum_d e (E (ea + eb) + 5) / (ea - eb) + (3 D + 2) e.
  sums   a workgroup adds its at most per_split terms in order, all positive, one rounding each (a multiply-add), and
         the splits are added in order: (min(m, per_split) + nsplit) e relative on the row's sum S_i.  The product with w
         inside the multiply-add costs nothing more; the prefactor (3 e) and the product with it (e).
  ln     one ulp of the result: 2 e |ln f_-i|.
  mean   m logarithms added in order on the host: (m - 1) e mean |ln f_-i|, and the division e.
With Q_i = sum_j t_ij q_ij / S_i and R_i = sum_j t_ij rho_j / S_i (the q and the weights' errors of the terms that carry
row i's sum, weighted as they carry it):
  bound = mean_i [(D + 4) e Q_i + R_i] + (6 + min(m, per_split) + nsplit) e + (m + 2) e mean_i |ln f_-i|.
This module's own scores are f64 arithmetic of the same shape with numpy's pairwise sums and a host erfc: they sit within
the same bound of the truth (tests/test_kde_cv_reference_cpu.py measures them against np.longdouble at small m), so a
comparison of the device with this module allows 2 * bound.

Candidates whose score is -inf here must be -inf on the device and the other way round: a row's sum is 0 when every
exp(-q) underflows to 0, and the tests keep such candidates far from the threshold (q of the nearest neighbour > 2000
against exp's 745)."""
import math

import numpy as np

from tests.kde_reference import _erfc

EPS = 2.0 ** -53
ERFC_ULPS = 16.0          # E of the module docstring, in units of EPS
MAX_CANDIDATES = 32
CV_SPLITS, CV_GRAIN, CV_PARTIALS = 16, 256, 1 << 22
PAIRS_PER_CHUNK = 1 << 21


# ------------------------------------------------------------------ kde_cv.h, restated
class Options:
    def __init__(self, lo=0.125, hi=4.0, steps=21, per_observable=True, max_rows=65536):
        self.lo, self.hi, self.steps, self.per_observable, self.max_rows = lo, hi, steps, per_observable, max_rows


def grid(lo, hi, steps):
    """s_k = lo (hi / lo)^(k / (steps - 1)) through log2 and 2^x, the ends lo and hi themselves."""
    if not (1 <= steps <= MAX_CANDIDATES):
        raise ValueError("Cross-validation steps must be between 1 and 32.")
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        raise ValueError("Cross-validation grid needs 0 < lo <= hi, both finite.")
    l0, l1 = math.log2(lo), math.log2(hi)
    s = [lo if steps == 1 else math.pow(2.0, l0 + ((l1 - l0) * k) / (steps - 1)) for k in range(steps)]
    s[0] = lo
    if steps > 1:
        s[-1] = hi
    return np.array(s)


def split(m, K):
    """(per_split, nsplit) of a scan of K candidates on m rows."""
    room = CV_PARTIALS // (max(m, 1) * max(K, 1))
    splits = min(CV_SPLITS, max(1, room))
    share = (m + splits - 1) // splits
    per_split = max(CV_GRAIN, (share + CV_GRAIN - 1) // CV_GRAIN * CV_GRAIN)
    return per_split, max(1, (m + per_split - 1) // per_split)


def subset(n, max_rows):
    """The in-domain rows scored (numbers in table order among the n in-domain rows)."""
    stride = 1 if (max_rows == 0 or n <= max_rows) else (n + max_rows - 1) // max_rows
    return np.arange(0, n, stride)


def choose(g, scores):
    """Index of the largest finite score; ties to the smaller |ln s|, then the smaller s; -1 when none is finite."""
    best = -1
    for c in range(len(g)):
        if not math.isfinite(scores[c]):
            continue
        if best < 0 or scores[c] > scores[best]:
            best = c
        elif scores[c] == scores[best]:
            a, b = abs(math.log(g[c])), abs(math.log(g[best]))
            if a < b or (a == b and g[c] < g[best]):
                best = c
    return best


def gap(scores):
    """How far the best finite score leads the runner-up (inf with fewer than two finite scores)."""
    f = np.sort(np.asarray(scores)[np.isfinite(scores)])
    return float(f[-1] - f[-2]) if len(f) >= 2 else math.inf


def search(options, D, scorer):
    """kde_cv.h's cv_search: scorer(mult [K, D]) -> scores [K].  A dict with the report's fields."""
    g = grid(options.lo, options.hi, options.steps)
    K = len(g)
    scale = np.ones(D)
    at_edge = [False] * D
    scans = []
    rep = dict(score_at_one=math.nan)
    for scan in range(1 + D if options.per_observable else 1):
        obs = scan - 1
        mult = np.tile(scale, (K, 1))
        if obs < 0:
            mult[:, :] = g[:, None]
        else:
            mult[:, obs] = g
        scores = np.asarray(scorer(mult), np.float64)
        c = choose(g, scores)
        if c < 0:
            raise ValueError("Cross-validation found no finite score: every candidate leaves some row without a "
                             "neighbour in reach (widen the grid upwards).")
        for d in range(D):
            if obs < 0 or d == obs:
                scale[d] = g[c]
                at_edge[d] = c in (0, K - 1)
        rep["score"] = float(scores[c])
        if obs < 0:
            for k in range(K):
                if g[k] == 1.0:
                    rep["score_at_one"] = float(scores[k])
        scans.append(dict(observable=obs, grid=g.copy(), scores=scores, chosen=c))
    rep.update(scale=scale, at_edge=at_edge, scans=scans)
    return rep


# ------------------------------------------------------------------ the rows
def scored_rows(samples, nfields, nobs, lower, upper, max_rows=0):
    """(x [m, D] f64, n, sigma [D]): the rows a scan scores, the in-domain count and the evaluator's own standard
    deviations over all n in-domain rows."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.all((x >= lower) & (x < upper), axis=1)
    s0 = x[inside]
    n = len(s0)
    sigma = np.array([math.sqrt(float(np.sum((s0[:, d] - s0[:, d].sum() / n) ** 2)) / (n - 1)) for d in range(nobs)])
    return s0[subset(n, max_rows)], n, sigma


def candidates(mult, sigma, m):
    """h_cd = s_cd sigma_d m^(-1/(D+4)): the candidates of a search on m rows."""
    D = len(sigma)
    return np.asarray(mult, np.float64) * np.asarray(sigma)[None, :] * float(m) ** (-1.0 / (D + 4))


# ------------------------------------------------------------------ the scores
def masses(x, h, lower, upper, dtype=np.float64):
    """(M [m, D], rho [m]): the truncation masses at bandwidths h, written as the contract writes them, and the bound
    on the relative error of the device's weight 1 / (prod h prod M) (module docstring)."""
    r = 1.0 / (np.asarray(h, np.float64) * math.sqrt(2.0))
    ea, eb = _erfc((x - upper) * r), _erfc((x - lower) * r)
    M = 0.5 * (ea - eb)
    D = x.shape[1]
    rho = (EPS * (ERFC_ULPS * (ea + eb) + 5.0) / (ea - eb)).sum(axis=1) + (3 * D + 2) * EPS
    return M.astype(dtype), rho


def scores(x, lower, upper, bandwidths, dtype=np.float64):
    """(score [K], bound [K]) of the candidates bandwidths [K, D] on the rows x [m, D].  dtype np.longdouble takes the
    pair sums, exp and ln in extended precision (the masses stay f64: numpy has no wider erfc)."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    x = np.asarray(x, np.float64)
    bw = np.asarray(bandwidths, np.float64).reshape(-1, x.shape[1])
    m, D = x.shape
    if m < 2:
        raise ValueError("Cross-validation needs at least 2 rows to score.")
    per_split, nsplit = split(m, len(bw))
    out, bound = np.empty(len(bw)), np.empty(len(bw))
    xx = x.astype(dtype)
    step = max(1, PAIRS_PER_CHUNK // m)
    for c, h in enumerate(bw):
        M, rho = masses(x, h, lower, upper, dtype)
        w = 1.0 / (np.prod(h.astype(dtype)) * np.prod(M, axis=1))
        g = 1.0 / (2.0 * h.astype(dtype) * h.astype(dtype))
        lnf, Q, R = np.empty(m, dtype), np.zeros(m), np.zeros(m)
        pref = 1.0 / (dtype(2.0 * math.pi) ** (D / 2.0) * (m - 1))
        for a in range(0, m, step):
            b = min(m, a + step)
            z = xx[a:b, None, :] - xx[None, :, :]
            q = (z * z * g).sum(axis=2)
            t = w[None, :] * np.exp(-q)
            t[np.arange(b - a), np.arange(a, b)] = 0.0          # the pair j == i is left out
            S = t.sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                lnf[a:b] = np.log(S * pref)
                Q[a:b] = np.where(S > 0, (t * q).sum(axis=1) / S, 0.0)
                R[a:b] = np.where(S > 0, (t * rho[None, :]).sum(axis=1) / S, 0.0)
        out[c] = float(lnf.sum() / m)
        if math.isfinite(out[c]):
            bound[c] = (float(np.mean((D + 4) * EPS * Q + R)) + (6 + min(m, per_split) + nsplit) * EPS
                        + (m + 2) * EPS * float(np.mean(np.abs(lnf))))
        else:
            bound[c] = 0.0
    return out, bound


def scores_double_loop(x, lower, upper, h):
    """score(h) by the contract's formulas one pair at a time (math.erfc, math.exp): for small m."""
    m, D = len(x), len(h)
    total = 0.0
    for i in range(m):
        f = 0.0
        for j in range(m):
            if j == i:
                continue
            term = 1.0
            for d in range(D):
                M = (0.5 * math.erfc((x[j][d] - upper[d]) / (h[d] * math.sqrt(2.0)))
                     - 0.5 * math.erfc((x[j][d] - lower[d]) / (h[d] * math.sqrt(2.0))))
                zz = (x[i][d] - x[j][d]) / h[d]
                term *= math.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi) / (h[d] * M)
            f += term
        f /= (m - 1)
        total += math.log(f) if f > 0 else -math.inf
    return total / m


def select(samples, nfields, nobs, lower, upper, options=None):
    """The search of sxmc_kde_cv_select on a table: the report (a dict) with rows_used."""
    o = options or Options()
    x, _, sigma = scored_rows(samples, nfields, nobs, lower, upper, o.max_rows)
    rep = search(o, nobs, lambda mult: scores(x, lower, upper, candidates(mult, sigma, len(x)))[0])
    rep["rows_used"] = len(x)
    return rep


# ------------------------------------------------------------------ the tables the tests share
def table(rng, n, D, outside=0.15, nfields=None):
    """[n, nfields] float32 rows: Gaussian blobs in the domain, rows outside it interleaved with rows inside, one row
    one float below `upper`, one on `lower`, and duplicated rows.  (samples, lower, upper)."""
    nfields = nfields or D
    lower = np.array([-1.0, 0.0, 2.0, -3.0][:D])
    upper = lower + np.array([4.0, 1.5, 6.0, 2.5][:D])
    mid, wid = (lower + upper) / 2, upper - lower
    x = np.zeros((n, nfields))
    x[:, :D] = mid + 0.18 * wid * rng.normal(size=(n, D))
    x[:, D:] = rng.normal(size=(n, nfields - D))
    x = x.astype(np.float32)
    out = rng.random(n) < outside
    out[:2] = False
    if n > 4:
        out[3] = True
    x[out, 0] = np.float32(upper[0]) + rng.random(int(out.sum())).astype(np.float32)
    x[0, :D] = np.nextafter(upper.astype(np.float32), np.float32(-np.inf))       # one float below upper
    if n > 2:
        x[2, :D] = lower.astype(np.float32)                                      # on lower: inside
    if n > 8:
        x[n - 1] = x[5]                                                          # duplicated rows
        x[n - 2] = x[5]
    return x, lower, upper


def table_with_inside(seed, m, D, nfields=None):
    """A table() cut after its m-th in-domain row: exactly m rows inside the domain, the last of them a duplicate of an
    earlier one."""
    rng = np.random.default_rng(seed)
    x, lower, upper = table(rng, m + m // 2 + 8, D, nfields=nfields)

    def inside(t):
        t = t[:, :D].astype(np.float64)
        return np.all((t >= lower) & (t < upper), axis=1)

    last = np.flatnonzero(inside(x))[m - 1]
    x = x[:last + 1].copy()
    if last > 8 and inside(x)[5]:
        x[last] = x[5]
    assert int(inside(x).sum()) == m
    return x, lower, upper


def two_peaks(seed, n=400):
    """Two peaks of sigma 0.1 at +-3 on [-10, 10): Scott's rule over-smooths them."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(n) < 0.5, -3.0, 3.0) + 0.1 * rng.normal(size=n)
    return x.astype(np.float32).reshape(-1, 1), np.array([-10.0]), np.array([10.0])


def unit_gaussian(seed, n=1000):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n).astype(np.float32).reshape(-1, 1), np.array([-10.0]), np.array([10.0])


def blob_2d(seed, n=500):
    """A 2-D sample narrow along one observable and bimodal along the other: the coordinate scans move off the
    common choice."""
    rng = np.random.default_rng(seed)
    a = np.where(rng.random(n) < 0.5, -2.0, 2.0) + 0.15 * rng.normal(size=n)
    b = rng.normal(size=n)
    x = np.stack([a, b, rng.normal(size=n)], axis=1).astype(np.float32)       # (a third field no observable reads)
    return x, np.array([-6.0, -6.0]), np.array([6.0, 6.0])


CONFIG_CV = dict(lo=0.125, hi=2.0, steps=9, max_rows=500)      # the "bandwidth_cv" of the configuration tests


def config_line_table(n=800):
    """The kernel signal of the configuration tests: a narrow line on a wide one, energy and true energy [n, 2]."""
    rng = np.random.default_rng(27)
    t = np.concatenate([rng.normal(6.0, 0.1, n // 2), rng.normal(6.0, 1.2, n - n // 2)])
    rng.shuffle(t)
    return np.stack([t + rng.normal(0, 0.05, n), t], axis=1).astype(np.float32)


def selection_cases():
    """name -> (samples [n, nfields], nobs, lower, upper, Options): the searches the GPU tests repeat.  Every scan of
    every one of them passes the gap condition (tests/test_kde_cv_reference_cpu.py asserts it)."""
    cases = {}
    x, lo, hi = two_peaks(11)
    cases["two_peaks_common"] = (x, 1, lo, hi, Options(per_observable=False, max_rows=0))
    x, lo, hi = unit_gaussian(12, 600)
    cases["gaussian"] = (x, 1, lo, hi, Options(max_rows=0))
    x, lo, hi = blob_2d(13)
    cases["blob_2d_per_observable"] = (x, 2, lo, hi, Options(lo=0.25, hi=4.0, steps=9, max_rows=0))
    cases["blob_2d_subset"] = (x, 2, lo, hi, Options(lo=0.25, hi=2.0, steps=7, max_rows=200))
    x, lo, hi = table(np.random.default_rng(14), 300, 3)
    cases["table_3d_narrow_grid"] = (x, 3, lo, hi, Options(lo=0.9, hi=1.1, steps=3, max_rows=0))
    cases["config_line"] = (config_line_table()[:, :1].copy(), 1, np.array([0.0]), np.array([10.0]),
                            Options(per_observable=True, **CONFIG_CV))
    return cases
