"""The contract of pdfz::EvalKernel's cutoff radius (include/sxmc_hip.h, sxmc_kde_set_cutoff) restated in numpy f64 on
top of tests/kde_reference.py and tests/kde_adaptive_reference.py: the envelope a value must lie in, and a numpy replay
of the visit test (sxmc_amd/csrc/kde_cutoff.h, cutoff_visit).  No device needed.

The envelope.  In the kernels' units (c = (x - lower) sqrt(log2(e) / 2) / h with the global h, a_d = c_pd - c_id,
q' = g sum_d a_d^2, g = 1 / lambda^2 or 1, a term t = W exp2(-q')) and with qcut = R^2 log2(e) / 2, per point:
  full = the contract value without a cutoff (every pair);
  kept = the same sum over the pairs with q' < qcut - dq, dq = 4 u c_max g sum_d |a_d| + (D + 5) u q' the bound of
         kde_adaptive_reference.py on the error of the kernel's own f32 q' (it covers the fixed kernel, whose bound is
         smaller): a pair the kernel may drop has f32 q' >= qcut, so its exact q' is >= qcut - dq, and every pair in
         `kept` is certainly summed.
The kernel sums a set V of pairs between the two, each term non-negative, so in exact arithmetic kept <= value <= full;
its f32 arithmetic on V errs by at most the existing rounding bound taken over ALL pairs (V's sums are no larger), with
the tile-position term u sum_i (256 - pos_i) t_i replaced by 256 u S0, which holds in any row order.  The check is
  kept - bound <= got <= full + bound.
(The device compares with qcut rounded UP to f32, which only adds pairs.)

The negative control: CutoffRef.culled is a numpy emulation (f64) of the culled sum with the pairs of q' in
[0.8 qcut, qcut) dropped as well; at R = 3 those terms are 1 to 3 % of a kernel height each, far above the bound, and the check must
fail (tests/test_kde_cutoff_reference_cpu.py verifies it on the CPU for the inputs the GPU tests use)."""
import math
from dataclasses import dataclass

import numpy as np

from tests.kde_adaptive_reference import mass_at, ref_local_factors
from tests.kde_reference import CSCALE, PAIRS_PER_CHUNK, TILE, U, ref_bandwidths, ref_transform

LOG2E_HALF = 0.72134752044448170
BOX, WAVE_BOX, WAVE = 9, 8, 64


def qcut_of(R):
    return math.inf if math.isinf(R) else R * R * LOG2E_HALF


def qcut_f32(R):
    """The f32 the kernels compare with: qcut rounded up."""
    q = qcut_of(R)
    if not q < float(np.finfo(np.float32).max):
        return np.float32(np.inf)
    f = np.float32(q)
    return f if float(f) >= q else np.nextafter(f, np.float32(np.inf))


@dataclass
class CutoffRef:
    full: np.ndarray     # f64 per point: every pair (NaN, 0 where the point codes say)
    kept: np.ndarray     # the pairs certainly below the cutoff
    bound: np.ndarray    # the rounding bound
    culled: np.ndarray   # emulate: the pairs with q' < also_drop * qcut, in f64
    norm: int
    c_max: float


def ref_cutoff(samples, nfields, nobs, lower, upper, scale, alpha, systs, params, points, R, dataset=0, also_drop=0.8,
               lam=None):
    """lam: the local factors of every table row as an INPUT (float64 [rows]) instead of ref_local_factors, whose cost
    grows as rows^2 -- for tables too large for it; only read when alpha > 0."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    D = nobs
    h = ref_bandwidths(samples, nfields, D, lower, upper, scale)
    nrows = np.asarray(samples).size // nfields
    if alpha > 0 and lam is not None:
        lam = np.array(lam, np.float64)
        assert lam.shape == (nrows,) and np.all(lam > 0)
    else:
        lam = ref_local_factors(samples, nfields, D, lower, upper, scale, alpha) if alpha > 0 else np.ones(nrows)
    s = ref_transform(samples, nfields, systs, params)[:, :D]
    with np.errstate(invalid="ignore"):
        inside = np.all((s >= lower) & (s < upper), axis=1)
    s, lam = s[inside], lam[inside]
    norm = int(inside.sum())
    W = 1.0 / mass_at(s, h[None, :] * lam[:, None], lower, upper) / lam ** D
    g = 1.0 / (lam * lam)
    pts = np.asarray(points, np.float32).reshape(-1, D + 1)
    x = pts[:, :D].astype(np.float64)
    with np.errstate(invalid="ignore"):
        in_dom = np.all((x >= lower) & (x < upper), axis=1)
    mine = in_dom & (pts[:, D] == np.float32(dataset))
    cs = CSCALE / h
    cx, cq = (x - lower) * cs, (s - lower) * cs
    c_max = float(max(np.abs(cq).max(initial=0.0), np.abs(cx[mine]).max(initial=0.0)))
    qcut = qcut_of(R)
    S = np.zeros((5, len(x)))
    step = max(1, PAIRS_PER_CHUNK // max(len(s) * D, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(x), step):
            b = min(len(x), a + step)
            A = cx[a:b, None, :] - cq[None, :, :]
            absA = np.abs(A).sum(axis=2)
            q = (A * A).sum(axis=2) * g[None, :]
            e = np.exp2(-q)
            dq = 4 * U * c_max * g[None, :] * absA + (D + 5) * U * q
            S[0, a:b] = e @ W
            S[1, a:b] = (e * absA) @ (W * g)
            S[2, a:b] = (e * q) @ W
            S[3, a:b] = np.where(q < qcut - dq, e, 0.0) @ W
            S[4, a:b] = np.where(q < also_drop * qcut, e, 0.0) @ W
    c = 1.0 / ((2 * math.pi) ** (D / 2) * np.prod(h))
    coef = D + 5 if alpha > 0 else D + 3
    with np.errstate(invalid="ignore", divide="ignore"):
        scale_ = c / norm if norm else np.nan
        full, kept, culled = S[0] * scale_, S[3] * scale_, S[4] * scale_
        bound = (c / norm if norm else 0.0) * (U * (math.log(2) * (4 * c_max * S[1] + coef * S[2]) + 3 * S[0]
                                                    + TILE * S[0]) + 2.0 ** -126 * W.sum())
    bound = bound + U * np.abs(np.nan_to_num(full)) + 2.0 ** -149
    for v in (full, kept, culled):
        v[in_dom & ~mine] = 0.0
        v[~in_dom] = np.nan
    return CutoffRef(full, kept, bound, culled, norm, c_max)


def inside_envelope(got, ref):
    """(ok, worst excess / bound): NaN exactly where the contract has NaN, kept - bound <= got <= full + bound
    elsewhere."""
    got = np.asarray(got, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(ref.full)):
        return False, math.inf
    ok = ~np.isnan(ref.full)
    over = got[ok] - ref.full[ok]
    under = ref.kept[ok] - got[ok]
    worst = float(np.max(np.maximum(over, under) / ref.bound[ok], initial=-math.inf))
    return worst <= 1.0, worst


def check_envelope(got, ref, label):
    ok, worst = inside_envelope(got, ref)
    live = ~np.isnan(ref.full) & (ref.full > 0)
    drop = float(np.max((ref.full[live] - ref.kept[live]) / ref.full[live], initial=0.0))
    print("%s: c_max %.4g, worst excess / bound %.3g, widest envelope %.3g of the value" % (label, ref.c_max, worst, drop))
    assert ok, "%s: outside the envelope by %.3g x the bound" % (label, worst)
    # the negative control: the sum that also drops [0.8 qcut, qcut) is outside
    bad, excess = inside_envelope(ref.culled, ref)
    print("%s control: the over-culled sum is outside by %.3g x the bound" % (label, excess))
    return worst, not bad


# ------------------------------------------------------------------ the visit test, replayed
def _f32_fma(a, b, c):
    """fmaf on float32 arrays: the product of two f32 is exact in f64, the sum rounds once to f64 and once to f32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def replay_visits(D, tile_boxes, wave_boxes, R):
    """[waves, tiles] bool: cutoff_visit of every wave box against every tile box, operation by operation in f32."""
    t, w = np.asarray(tile_boxes, np.float32), np.asarray(wave_boxes, np.float32)
    zero = np.float32(0.0)
    q = None
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            a = t[None, :, d] - w[:, None, 4 + d]
            b = w[:, None, d] - t[None, :, 4 + d]
            gap = np.where(a > b, a, b)
            gap = np.where(gap > zero, gap, zero).astype(np.float32)
            q = gap * gap if d == 0 else _f32_fma(gap, gap, q)
        q = (t[None, :, 8] * q).astype(np.float32)
    return q < qcut_f32(R)


# ------------------------------------------------------------------ the inputs of the cutoff tests
LOWER, UPPER = np.array([0.5, 0.0, 2.0, 1.0]), np.array([8.5, 3.0, 11.0, 7.0])
SIZES = (255, 256, 257, 1000)          # sample rows: around one tile, and several tiles
POINTS = (1, 63, 64, 65, 300)          # points: around one wave, and more than one workgroup
PARAMS = {0: 0.03, 1: 0.5, 2: 0.1}     # shift, scale (x 1.5), resolution


def cutoff_systs(D):
    """Shift and resolution on observable 0, scale on the last: the moved samples' boxes are not the order's."""
    return [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=D - 1, pars=[1]),
            dict(type="resolution_scale", obs=0, true_obs=D, pars=[2])]


def cutoff_table(D, N, rng, first_tile_outside=False):
    """(samples, nfields, lower, upper): three narrow clusters on a thin floor, placed so that the nominal systematics
    (PARAMS) keep most rows inside the domain and move some across its edges; one truth field."""
    lower, upper = LOWER[:D], UPPER[:D]
    wid = upper - lower
    which = rng.integers(0, 3, N)
    y = lower + wid * (np.array([0.2, 0.5, 0.8])[which][:, None] + 0.04 * rng.normal(size=(N, D)))
    floor = rng.random(N) < 0.1
    y[floor] = lower + wid * rng.uniform(-0.05, 1.05, (int(floor.sum()), D))
    x = y.copy()
    x[:, D - 1] = x[:, D - 1] / 1.5
    if first_tile_outside:
        x[:TILE, 0] = (lower[0] - rng.uniform(0.0, 0.3, TILE)) / (1.5 if D == 1 else 1.0)
    truth = x[:, 0] + 0.02 * wid[0] * rng.normal(size=N)
    return np.concatenate([x, truth[:, None]], axis=1).astype(np.float32).ravel(), D + 1, lower, upper


def cutoff_points(D, E, rng, lower, upper):
    """E points over a little more than the domain; from the second on, one outside it and one of another data set."""
    wid = upper - lower
    p = np.zeros((E, D + 1))
    p[:, :D] = lower + wid * rng.uniform(-0.03, 1.03, (E, D))
    p[0, :D] = lower + 0.5 * wid
    if E > 1:
        p[1, 0] = upper[0] + 0.1
    if E > 2:
        p[2, :D] = lower + 0.21 * wid
        p[2, D] = 1.0
    return p.astype(np.float32).ravel()


# The shapes at which a workgroup of the culled pair sum walks many tiles (tests/test_gpu_kde_cutoff_splits.py):
# (points, sample rows), the smallest at which kde_plan.h's pair_split followed by kde_cutoff.h's cutoff_split gives,
# on 256 compute units, the split named -- which the GPU tests read back from the evaluator, not from here.
REGIMES = {
    "A": (16384, 24700),       # (25, 4): several bits in one ballot; the last split holds 1 tile of 4
    "A'": (16384, 130000),     # (32, 16): 16 bits; the last split holds 12
    "B1": (524188, 17000),     # (1, 67): two rounds of 64 tiles, the second with 3 lanes
    "B2": (262144, 35000),     # (2, 69): two rounds in each split; the second split clipped to 68
    "C1": (100000, 10400),     # plain (41, 1) becomes (21, 2): cutoff_split doubles; the last split holds 1
    "C2": (100000, 131072),    # plain 2 tiles per split becomes (32, 16): the doubling taken three times
}
SUBSAMPLE = 1024               # at most this many of the caller's points are compared
PAIRS_PER_CASE = 2.5e7         # ... and about this many pairs, so that a case's reference takes a few seconds


def regime_inputs(name, D, rows=None):
    """(samples, nfields, lower, upper, points) of a regime at D observables; rows: a smaller table from the same
    generator (the points stay the same: they have a generator of their own)."""
    npts, nrows = REGIMES[name]
    seed = 8800 + 10 * sorted(REGIMES).index(name) + D
    samples, nf, lower, upper = cutoff_table(D, nrows if rows is None else rows, np.random.default_rng(seed))
    return samples, nf, lower, upper, cutoff_points(D, npts, np.random.default_rng(seed + 100), lower, upper)


def strided(npts, nrows=0):
    """The places of the caller's points that are compared: the three special points of cutoff_points, every stride-th
    from the first, and the last -- at most SUBSAMPLE of them, fewer against a table of many rows."""
    if npts <= SUBSAMPLE:
        return np.arange(npts)
    want = int(min(SUBSAMPLE, max(128, PAIRS_PER_CASE // max(nrows, 1)))) - 3
    stride = -(-npts // want)
    idx = np.unique(np.concatenate([[0, 1, 2, npts - 1], np.arange(0, npts, stride)]))
    assert len(idx) <= SUBSAMPLE and idx[-1] == npts - 1
    return idx


def clip_table(N=1000):
    """2-D, for sensitivity 1 at bandwidth scale 0.3: a narrow line on a broad bump on a flat floor -- the line's rows
    clip at lambda 0.1, the floor's at 10."""
    rng = np.random.default_rng(9)
    lower, upper = LOWER[:2], UPPER[:2]
    wid, mid = upper - lower, (lower + upper) / 2
    n1, n3 = N // 5, N // 25
    x = np.concatenate([mid + 0.004 * wid * rng.normal(size=(n1, 2)), mid + 0.06 * wid * rng.normal(size=(N - n1 - n3, 2)),
                        rng.uniform(lower, upper, (n3, 2))])
    x = x[rng.permutation(N)]
    return x.astype(np.float32).ravel(), 2, lower, upper
