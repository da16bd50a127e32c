"""pdfz::EvalKernel over WEIGHTED Monte Carlo samples (sxmc_kde_create_weighted, the laws in include/sxmc_hip.h) restated
in numpy f64 with integers: the reference of the weighted kernel-density tests.  No device needed.  TEST INFRASTRUCTURE.

A table row carries an integer multiplicity m_i.  Everything below is tests/kde_reference.py, kde_adaptive_reference.py,
kde_cutoff_reference.py and kde_sample_reference.py with every term carrying m_i:

  bandwidths  law_bandwidths(): the law operation by operation in Python floats and integers (sequential sums, one
              rounding per operation) -- what sxmc_amd/csrc/kde_weights.h is held to bit for bit.  ref_kde_weighted()
              computes its own h with numpy's sums, as kde_reference.ref_bandwidths does (with all m = 1 the same bytes
              as that), or takes h as an input.
  evaluation  norm = sum m_i over the moved in-domain rows; W_i = m_i / (mass_i lambda_i^D); the value and the bound are
              kde_reference's (kde_adaptive_reference's when alpha > 0) with W_i for w_i.  With R > 0 also the envelope
              of kde_cutoff_reference: `kept`, the pairs certainly below the cutoff, and the bound with the whole tile.
  pilot       f_i = c / S1 sum_j (m_j / mass_j) prod phi(...) over the in-domain rows; g = exp(sum m_i ln f_i / S1) over
              the in-domain rows with m_i > 0; lambda as kde_adaptive_reference.
  projection  share_j = (1 / norm) sum_i m_i [...].
  sampling    T = norm; C = the inclusive prefix sums of the multiplicities of the live rows (in domain, m > 0) in table
              order; an attempt's first word picks target = (word * T) >> 32 and the first live row whose C exceeds it.
              draw_weighted() replays an event stream with kde_sample_reference.draw, the pick replaced by this law.

PLANTS / PICK_PLANTS: references wrong on purpose, one way at a time (the negative controls)."""
import contextlib
import math
from dataclasses import dataclass

import numpy as np

from tests import kde_sample_reference as KS
from tests.kde_adaptive_reference import LAMBDA_MAX, LAMBDA_MIN, mass_at
from tests.kde_cutoff_reference import qcut_of
from tests.kde_reference import CSCALE, PAIRS_PER_CHUNK, TILE, U, phi, ref_transform

PLANTS = ("norm_unweighted", "sum_unweighted", "m_squared", "n_for_neff")
PICK_PLANTS = ("uniform", "first_ge")


# ------------------------------------------------------------------ the bandwidth law, operation by operation
def _inside(x, lower, upper):
    with np.errstate(invalid="ignore"):
        return np.all((x >= lower) & (x < upper), axis=1)


def law_bandwidths(samples, nfields, nobs, lower, upper, scale, m=None, plant=None):
    """dict(s1, s2, n_eff, mean, sigma, h, live) or raises ValueError naming the refusal.  m None: every row once."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    rows = np.flatnonzero(_inside(x, lower, upper))
    mm = [1] * len(x) if m is None else [int(v) for v in np.asarray(m).reshape(-1)]
    S1 = sum(mm[i] for i in rows)                      # exact integers
    S2 = sum(mm[i] * mm[i] for i in rows)
    live = sum(1 for i in rows if mm[i] > 0)
    s1, s2 = float(S1), float(S2)                      # int -> float rounds to nearest even, once
    out = dict(s1=s1, s2=s2, live=live)
    if live < 2:
        raise ValueError("too few")
    n_eff = s1 * (s1 / s2)
    if plant == "n_for_neff":
        n_eff = float(len(rows))
    freedom = s1 - s2 / s1
    if not freedom > 0.0:
        raise ValueError("no freedom")
    mean, sigma, h = [], [], []
    for d in range(nobs):
        acc = 0.0
        for i in rows:
            acc = acc + float(mm[i]) * float(x[i, d])
        mu = acc / s1
        v = 0.0
        for i in rows:
            dx = float(x[i, d]) - mu
            v = v + float(mm[i]) * (dx * dx)
        sg = math.sqrt(v / freedom)
        if not sg > 0.0:
            raise ValueError("no spread %d" % d)
        mean.append(mu)
        sigma.append(sg)
        h.append((float(scale[d]) * sg) * math.pow(n_eff, -1.0 / (nobs + 4)))
    out.update(n_eff=n_eff, mean=np.array(mean), sigma=np.array(sigma), h=np.array(h))
    return out


def ref_weighted_bandwidths(samples, nfields, nobs, lower, upper, scale, m, plant=None):
    """(h, n_eff, s1): the same law with numpy's sums (kde_reference.ref_bandwidths' operations when all m = 1)."""
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    inside = _inside(x, np.asarray(lower, np.float64), np.asarray(upper, np.float64))
    mi = np.asarray(m, np.float64).reshape(-1)[inside]
    xi = x[inside]
    s1, s2 = float(mi.sum()), float((mi * mi).sum())
    n_eff = float(inside.sum()) if plant == "n_for_neff" else s1 * (s1 / s2)
    mu = (xi * mi[:, None]).sum(axis=0) / s1
    dx = xi - mu
    sigma = np.sqrt((dx * dx * mi[:, None]).sum(axis=0) / (s1 - s2 / s1))
    return np.asarray(scale) * sigma * n_eff ** (-1.0 / (nobs + 4)), n_eff, s1


def repeated_table(samples, nfields, m):
    """The table in which row i stands m_i times, in table order."""
    t = np.asarray(samples, np.float32).reshape(-1, nfields)
    return np.repeat(t, np.asarray(m, np.int64).reshape(-1), axis=0)


# ------------------------------------------------------------------ the pilot
def ref_weighted_factors(samples, nfields, nobs, lower, upper, h, m, alpha):
    """lambda of every table row (f64 [rows]) of a weighted adaptive evaluator with bandwidths h."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    x = np.asarray(samples, np.float32).reshape(-1, nfields)[:, :nobs].astype(np.float64)
    inside = _inside(x, lower, upper)
    mi = np.asarray(m, np.float64).reshape(-1)
    s0 = x[inside]
    w = mi[inside] / mass_at(s0, np.broadcast_to(h, s0.shape), lower, upper)
    s1 = float(mi[inside].sum())
    f = np.empty(len(x))
    step = max(1, PAIRS_PER_CHUNK // max(len(s0) * nobs, 1))
    c = 1.0 / ((2 * math.pi) ** (nobs / 2) * np.prod(h))
    with np.errstate(invalid="ignore"):
        for a in range(0, len(x), step):
            z = (x[a:a + step, None, :] - s0[None, :, :]) / h
            f[a:a + step] = np.exp(-0.5 * (z * z).sum(axis=2)) @ w
    f = f * c / s1
    counted = inside & (mi > 0)
    g = math.exp(float(np.sum(mi[counted] * np.log(f[counted]))) / s1)
    good = np.isfinite(f) & (f > 0)
    lam = np.full(len(f), LAMBDA_MAX)
    with np.errstate(over="ignore"):
        lam[good] = np.minimum(LAMBDA_MAX, np.maximum(LAMBDA_MIN, (f[good] / g) ** (-alpha)))
    return lam


# ------------------------------------------------------------------ the values
@dataclass
class WeightedRef:
    values: np.ndarray   # f64 pdf per point (NaN, 0 where the point codes say); with R > 0 the sum over every pair
    norm: int
    h: np.ndarray
    bound: np.ndarray    # per point: the kernels' error bound with weighted terms
    c_max: float
    lam: np.ndarray      # [rows] the local factors (ones when alpha = 0)
    q_max: float         # the largest q' = g sum_d (c_pd - c_id)^2 over the compared points and the live rows
    full: np.ndarray = None   # (R > 0) = values
    kept: np.ndarray = None   # (R > 0) the pairs certainly below the cutoff


def ref_kde_weighted(samples, nfields, nobs, lower, upper, scale, systs, params, points, m, dataset=0, alpha=0.0, R=0.0,
                     h=None, plant=None):
    """The weighted contract in f64, chunked.  h: the bandwidths as an input (else the law's, by numpy's sums)."""
    assert plant is None or plant in PLANTS
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    D = nobs
    m = np.asarray(m, np.int64).reshape(-1)
    if h is None:
        h, _, _ = ref_weighted_bandwidths(samples, nfields, D, lower, upper, scale, m, plant)
    h = np.asarray(h, np.float64)
    nrows = np.asarray(samples).size // nfields
    lam = ref_weighted_factors(samples, nfields, D, lower, upper, h, m, alpha) if alpha > 0 else np.ones(nrows)
    s = ref_transform(samples, nfields, systs, params)[:, :D]
    inside = _inside(s, lower, upper)
    pos = np.flatnonzero(inside) % TILE
    s, lam_in, mi = s[inside], lam[inside], m[inside].astype(np.float64)
    norm = int(inside.sum()) if plant == "norm_unweighted" else int(m[inside].sum())
    msum = np.ones(len(s)) if plant == "sum_unweighted" else mi * mi if plant == "m_squared" else mi
    W = msum / mass_at(s, h[None, :] * lam_in[:, None], lower, upper) / lam_in ** D
    g = 1.0 / (lam_in * lam_in)
    pts = np.asarray(points, np.float32).reshape(-1, D + 1)
    x = pts[:, :D].astype(np.float64)
    in_dom = _inside(x, lower, upper)
    mine = in_dom & (pts[:, D] == np.float32(dataset))
    cs = CSCALE / h
    cx, cq = (x - lower) * cs, (s - lower) * cs
    c_max = float(max(np.abs(cq).max(initial=0.0), np.abs(cx[mine]).max(initial=0.0)))
    qcut = qcut_of(R) if R > 0 else math.inf
    S = np.zeros((5, len(x)))
    Wt = W * (TILE - pos)
    q_max = 0.0
    step = max(1, PAIRS_PER_CHUNK // max(len(s) * D, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(x), step):
            b = min(len(x), a + step)
            A = cx[a:b, None, :] - cq[None, :, :]
            absA = np.abs(A).sum(axis=2)
            q = (A * A).sum(axis=2) * g[None, :]
            e = np.exp2(-q)
            S[0, a:b] = e @ W
            S[1, a:b] = (e * absA) @ (W * g)
            S[2, a:b] = (e * q) @ W
            S[3, a:b] = e @ Wt
            if R > 0:
                dq = 4 * U * c_max * g[None, :] * absA + (D + 5) * U * q
                S[4, a:b] = np.where(q < qcut - dq, e, 0.0) @ W
            live = q[mine[a:b]][:, W > 0]
            if live.size:
                q_max = max(q_max, float(np.max(live)))
    c = 1.0 / ((2 * math.pi) ** (D / 2) * np.prod(h))
    coef = D + 5 if alpha > 0 else D + 3
    tile = TILE * S[0] if R > 0 else S[3]              # (sorted rows: a row's place in its tile is not the table's)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = S[0] * c / norm if norm else np.full(len(x), np.nan)
        kept = S[4] * c / norm if norm else np.full(len(x), np.nan)
        bound = (c / norm if norm else 0.0) * (U * (math.log(2) * (4 * c_max * S[1] + coef * S[2]) + 3 * S[0] + tile)
                                               + 2.0 ** -126 * W.sum())
    bound = bound + U * np.abs(np.nan_to_num(out)) + 2.0 ** -149
    for v in (out, kept):
        v[in_dom & ~mine] = 0.0
        v[~in_dom] = np.nan
    return WeightedRef(out, norm, h, bound, c_max, lam, q_max, out if R > 0 else None, kept if R > 0 else None)


# ------------------------------------------------------------------ the projection
def ref_weighted_marginal(samples, nfields, nobs, lower, upper, h, lam, systs, params, m, obs, nbins, plant=None):
    """shares [nbins] of sxmc_kde_project on a weighted evaluator with bandwidths h and factors lam [rows]; u through
    the prepass's f32 scaled coordinate, as the device reads it."""
    from tests.project_reference import bin_edges_t
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    m = np.asarray(m, np.int64).reshape(-1)
    s = ref_transform(samples, nfields, systs, params)[:, :nobs]
    live = _inside(s, lower, upper) & (m > 0)
    mi = m[live].astype(np.float64)
    norm = float(mi.sum())
    if plant == "sum_unweighted":
        mi = np.ones(len(mi))
    if plant == "norm_unweighted":
        norm = float(live.sum())
    lam = np.asarray(lam, np.float64)[live]
    u = ((s[live, obs] - lower[obs]) * (CSCALE / h[obs])).astype(np.float32).astype(np.float64) / CSCALE
    t = bin_edges_t(lower[obs], upper[obs], h[obs], nbins)
    mass = phi((t[-1] - u) / lam) - phi(-u / lam)
    cdf = phi((t[:, None] - u[None, :]) / lam[None, :])
    return ((cdf[1:] - cdf[:-1]) * (mi / mass)[None, :]).sum(axis=1) / norm


# ------------------------------------------------------------------ the sampler
def pick_places(word, cum, plant=None):
    """The place in the list of live rows an attempt's first word picks.  cum: the inclusive prefix sums of the live
    rows' multiplicities (Python ints or uint64, the last one T <= 2^32 - 1)."""
    assert plant is None or plant in PICK_PLANTS
    cum = np.asarray(cum, np.uint64)
    word = np.asarray(word, np.uint64)
    if plant == "uniform":
        return ((word * np.uint64(len(cum))) >> np.uint64(32)).astype(np.int64)
    target = (word * cum[-1]) >> np.uint64(32)          # < 2^64: word < 2^32, T < 2^32
    return np.searchsorted(cum, target, side="left" if plant == "first_ge" else "right").astype(np.int64)


@contextlib.contextmanager
def _weighted_pick(cum, plant):
    """While it holds, kde_sample_reference.draw picks by the weighted law: the first word of every attempt is replaced
    by the smallest word whose uniform pick over the len(cum) live rows is the place the law picks."""
    plain = KS.words
    n = len(cum)

    def words(event, counter, seed):
        A = list(plain(event, counter, seed))
        if np.all(np.asarray(counter) % 2 == 0):        # (block A of an attempt: its x picks the row)
            place = np.minimum(pick_places(A[0], cum, plant), n - 1)
            A[0] = np.array([-((-int(p) << 32) // n) for p in place], dtype=np.uint64)
        return tuple(A)

    KS.words = words
    try:
        yield
    finally:
        KS.words = plain


def prepare_weighted(table, nfields, nobs, lower, upper, h, m, systs=(), params=()):
    """kde_sample_reference.prepare over the LIVE rows (in domain after the systematics, m > 0), and the inclusive prefix
    sums of their multiplicities: (rows_c, row_index, fragile, cum)."""
    rows_c, row_index, fragile = KS.prepare(table, nfields, nobs, lower, upper, h, systs, params)
    mi = np.asarray(m, np.uint64).reshape(-1)[row_index]
    keep = mi > 0
    return rows_c[keep], row_index[keep], fragile[keep], np.cumsum(mi[keep], dtype=np.uint64)


def draw_weighted(rows_c, row_index, cum, lam, h, lower, upper, nevents, seed, lowers=None, uppers=None, dataset=0,
                  fragile=None, plant=None):
    """kde_sample_reference.draw with the weighted pick (its dict; its rules for ambiguous draws)."""
    with _weighted_pick(cum, plant):
        return KS.draw(rows_c, row_index, lam, h, lower, upper, nevents, seed, lowers, uppers, dataset, None, fragile)


# ------------------------------------------------------------------ the inputs the CPU and the GPU tests share
PARAMS = {0: 0.05, 1: 0.03, 2: 0.1}     # shift, scale, resolution: some rows cross the domain's edge
SHAPES = ((1, 255, 1), (2, 256, 63), (3, 257, 64), (4, 1023, 65), (2, 1025, 300), (1, 1023, 300))   # (D, N, E)
Q_LIMIT = 100.0                         # every pair's q' below this: no term or running sum is subnormal


@dataclass
class Case:
    D: int
    nfields: int
    table: np.ndarray     # float32 [N, nfields]: D observables, then the truth of observable 0
    lower: np.ndarray
    upper: np.ndarray
    scale: np.ndarray
    systs: list
    points: np.ndarray    # float32 [E, D + 1]
    dataset: int = 3


def case(D, N, E, seed=0):
    """A table around 0 with unit spread on a domain of +-2 sigma, bandwidth scale 2 (D <= 2) or 3: every pair's q' stays
    under Q_LIMIT (asserted on the reference by the tests).  Points: inside the domain, the last few outside it or of
    another data set when there is room."""
    rng = np.random.default_rng(1000 * D + N + 7 * E + seed)
    nfields = D + 1
    t = rng.normal(0.0, 1.0, (N, nfields))
    t[:, D] = t[:, 0] + rng.normal(0.0, 0.2, N)
    lower, upper = np.full(D, -2.0), np.full(D, 2.0)
    pts = np.empty((E, D + 1), np.float32)
    pts[:, :D] = rng.uniform(-1.95, 1.95, (E, D))
    pts[:, D] = 3
    if E >= 8:
        pts[-1, 0] = 2.5
        pts[-2, D] = 4
        pts[-3, 0] = np.nan
    systs = [dict(type="shift", obs=D - 1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
             dict(type="resolution_scale", obs=0, true_obs=D, pars=[2])]
    return Case(D, nfields, t.astype(np.float32), lower, upper, np.full(D, 2.0 if D <= 2 else 3.0), systs, pts)


def small_multiplicities(c, seed=1):
    """m in {0..3} with zeros on the first and the last row inside the domain (before and after the systematics) and,
    where the table has more than two tiles' rows, on the whole second 256-row tile."""
    rng = np.random.default_rng(seed + len(c.table))
    m = rng.integers(0, 4, len(c.table)).astype(np.uint32)
    for systs in ((), c.systs):
        s = ref_transform(c.table, c.nfields, list(systs), PARAMS)[:, :c.D]
        rows = np.flatnonzero(_inside(s, c.lower, c.upper))
        m[rows[0]] = m[rows[-1]] = 0
    if len(c.table) > 2 * TILE:
        m[TILE:2 * TILE] = 0
    return m


def spatial_order(table, D, lower, upper):
    """The order a cutoff puts the table rows in (sxmc_amd/csrc/kde_cutoff.h, cutoff_key and cutoff_order), restated:
    order[k] = the row that comes k-th.  One observable: the coordinate clamped to [lower, upper] (NaN counts as lower),
    a plain sort; more: the Morton code of the cell of a grid of 2^(32 // D) cells per observable over the domain,
    observable 0 the most significant within a bit level.  Stable, ties by table index."""
    x = np.asarray(table, np.float32)[:, :D].astype(np.float64)
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    if D == 1:
        v = np.where(x[:, 0] >= lower[0], x[:, 0], lower[0])
        return np.argsort(np.where(v > upper[0], upper[0], v).astype(np.float32), kind="stable")
    bits = 32 // D
    ncell = 1 << bits
    t = (x - lower) / (upper - lower)
    t = np.where(t >= 0.0, t, 0.0)
    t = np.where(t > 1.0, 1.0, t)
    cell = np.minimum(np.floor(t * float(ncell)), ncell - 1).astype(np.uint64)
    key = np.zeros(len(x), np.uint64)
    for b in range(bits - 1, -1, -1):
        for d in range(D):
            key = (key << np.uint64(1)) | ((cell[:, d] >> np.uint64(b)) & np.uint64(1))
    return np.argsort(key, kind="stable")
