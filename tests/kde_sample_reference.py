"""The kernel-density event sampler (sxmc_kde_random_sample: kde_flag / scan / kde_scatter and kde_sample_kernel of
sxmc_amd/csrc/kde_kernels.hip, the host side in sxmc_kde_draw.cpp) restated in numpy with integers and f64, vectorised
over events; the cases the CPU and the GPU tests share.

The contract (include/sxmc_hip.h, the comment of sxmc_kde_random_sample), statement for statement as the kernel has it:

  rows      the in-domain rows of the last evaluation in table order; row j of them holds, per observable, the float
            c = (float)((x - lower) * (KLOG / h)), x the f64 transform of the float table (what kde_prepass stores)
  words     event e, attempt t: block A = Philox4x32-10 with counter words (e lo, e hi, 2t, 0), block B with
            (e lo, e hi, 2t + 1, 0), key (seed lo, seed hi)
  row       A.x picks position (A.x * n) >> 32 of the n in-domain rows
  words     the coordinate words are A.y, A.z, A.w, B.x for observables 0..3
  centre    s = lower + (double)c * (h / KLOG), hw = h * lam[table row]
  mass      pa = Phi((lower - s) / hw), qb = Phi((s - upper) / hw), m = (0.5 - pa) + (0.5 - qb),
            Phi(z) = 0.5 * erfc(-z * 0.70710678118654752)
  inverse   p = pa + (u + 0.5) * 2^-32 * m; p <= 0.5: z = -SQRT2 * erfcinv(2 p); otherwise
            q = qb + ((2^32 - 1 - u) + 0.5) * 2^-32 * m and z = +SQRT2 * erfcinv(2 q)
  value     xd = s + hw * z, every operation rounded in f64
  float     xf = (float)xd; xf = bottom if not (xf >= lower); then xf = top if not (xf < upper) (f64 on the float;
            bottom the smallest float >= lower, top the largest float < upper)
  cuts      on the floats, inclusive: while xf > hi or xf < lo in any observable the event takes attempt t + 1 (a new
            row, new coordinates); an event that has not passed after ATTEMPTS attempts is exhausted

Phi and erfcinv are scipy.special's in f64.  The device's are its own library's, so its xd can differ from this one's in
the last bits and round to the neighbouring float.  draw() therefore flags a coordinate as AMBIGUOUS when its xd lies
within delta = 2^-40 * max(|xd|, hw) of a midpoint between two adjacent floats, of lower or upper, or of a cut bound;
an event that picks a FRAGILE row (prepare(): one whose f64 coordinate lies within 2^-40 relative of a float midpoint)
is ambiguous as a whole, and so is one that came near a cut bound in any of its attempts.  delta: the f64 replay was
measured within 10.8 * 2^-53 * max(|xd|, hw) of 60-digit arithmetic (tests/test_kde_sample_reference_cpu.py asserts 64),
so delta leaves about 750 times that to the device's two library calls.

`variant` makes draw() wrong on purpose, one way at a time: the negative controls of
tests/test_kde_sample_reference_cpu.py."""
import numpy as np
from scipy.special import erfc, erfcinv

from tests.hist_sample_reference import U32, domain_floats, words
from tests.kde_reference import ref_transform

ATTEMPTS = 1024
KLOG = 0.84932180028801907           # kLog2eHalfSqrt (sxmc_kde_state.h)
SQRT2 = 1.4142135623730950           # kde_phi_inv's literal (the double below sqrt 2)
SQRT_HALF = 0.70710678118654752      # kde_phi's literal
TWO_M32 = 2.3283064365386963e-10     # 2^-32
DELTA = 2.0 ** -40
VARIANTS = ("lam_by_position", "scatter_off_by_one", "reuse_word", "row_from_y", "single_counter", "seed_low_only",
            "one_minus_p", "clamp_before_round")


def phi(z):
    """kde_phi."""
    return 0.5 * erfc(-z * SQRT_HALF)


def point(c, factor, word, h, lower, upper, variant=None):
    """One coordinate: (xd, hw) from the row's scaled float c, its bandwidth factor, the coordinate word (arrays), and
    the observable's bandwidth and bounds (scalars).  centre .. value of the module docstring."""
    u = np.asarray(word).astype(np.float64)
    s = lower + np.asarray(c, np.float32).astype(np.float64) * (h / KLOG)
    hw = h * np.asarray(factor, np.float64)
    pa = phi((lower - s) / hw)
    qb = phi((s - upper) / hw)
    m = (0.5 - pa) + (0.5 - qb)
    p = pa + ((u + 0.5) * TWO_M32) * m
    if variant == "one_minus_p":
        q = 1.0 - p
    else:
        q = qb + (((4294967295.0 - u) + 0.5) * TWO_M32) * m
    low = p <= 0.5
    z = np.where(low, -SQRT2 * erfcinv(2.0 * np.where(low, p, 0.5)), SQRT2 * erfcinv(2.0 * np.where(low, 0.5, q)))
    xd = s + hw * z
    return xd, np.broadcast_to(hw, xd.shape)


def end_floats(lower, upper):
    """(bottom, top): the smallest float >= lower and the largest float < upper, as sxmc_kde_draw.cpp finds them."""
    return domain_floats(type("G", (), dict(lower=np.array([lower], np.float64), upper=np.array([upper], np.float64))), 0)


def midpoint_distance(xd):
    """|xd - the nearer of the two midpoints between (float)xd and its float neighbours| (f64, exact midpoints)."""
    xd = np.asarray(xd, np.float64)
    xf = xd.astype(np.float32)
    x = xf.astype(np.float64)
    up = np.nextafter(xf, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(xf, np.float32(-np.inf)).astype(np.float64)
    return np.minimum(np.abs(xd - (x + up) / 2), np.abs(xd - (x + dn) / 2))


def prepare(table, nfields, nobs, lower, upper, h, systs=(), params=()):
    """What kde_prepass leaves for the sampler: (rows_c float32 [n, D], row_index int64 [n], fragile bool [n]) of the
    in-domain rows in table order, from the f64 transform of the float table (tests/kde_reference.ref_transform: the
    IEEE operations of apply_op for one-coefficient systematics, in the order attached)."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = np.asarray(h, np.float64)
    f = ref_transform(table, nfields, list(systs), params)[:, :nobs]
    inside = np.all((f >= lower) & (f < upper), axis=1)
    v = (f[inside] - lower) * (KLOG / h)
    fragile = np.any(midpoint_distance(v) <= DELTA * np.abs(v), axis=1)
    return v.astype(np.float32), np.flatnonzero(inside).astype(np.int64), fragile


def draw(rows_c, row_index, lam, h, lower, upper, nevents, seed, lowers=None, uppers=None, dataset=0, variant=None,
         fragile=None):
    """The sampler.  Returns a dict:
      events float32 [n, D + 1]; row int64 [n] (the table row picked); attempts int64 [n] (1 .. ATTEMPTS); exhausted
      (how many events passed no attempt: the device call then fails); xd float64 [n, D]; scale float64 [n, D]
      (max(|xd|, hw): delta = DELTA * scale); mid float64 [n, D] (distance of xd to the nearest float midpoint);
      ambiguous bool [n, D] (xd within delta of a float midpoint, lower or upper); at_cut bool [n] (within delta of a cut
      bound -- or ambiguous on a float next to one -- in any attempt, or drawn from a fragile row: ambiguous as a whole);
      clamped_bottom, clamped_top (how many accepted coordinates took either clamp)."""
    assert variant is None or variant in VARIANTS
    rows_c = np.asarray(rows_c, np.float32)
    n, D = rows_c.shape
    assert n >= 1 and 1 <= D <= 4
    row_index = np.asarray(row_index, np.int64)
    lam = np.asarray(lam, np.float64)
    h = np.asarray(h, np.float64).reshape(-1)
    lower, upper = np.asarray(lower, np.float64).reshape(-1), np.asarray(upper, np.float64).reshape(-1)
    fragile = np.zeros(n, bool) if fragile is None else np.asarray(fragile, bool)
    if variant == "scatter_off_by_one":
        # the carry into the second 256-row block one short: every later row lands one place early, over the last row of
        # the first block, which is never picked; the last place keeps its row, which is picked twice
        early = np.flatnonzero(row_index >= 256)
        early = early[early > 0]
        rows_c, row_index = rows_c.copy(), row_index.copy()
        rows_c[early - 1], row_index[early - 1] = rows_c[early], row_index[early]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if variant == "seed_low_only":
        seed &= 0xFFFFFFFF
    ends = [end_floats(lower[k], upper[k]) for k in range(D)]
    has_cuts = lowers is not None
    if has_cuts:
        cut_lo, cut_hi = np.asarray(lowers, np.float32), np.asarray(uppers, np.float32)
    N = int(nevents)
    out = dict(events=np.zeros((N, D + 1), np.float32), row=np.zeros(N, np.int64), attempts=np.zeros(N, np.int64),
               xd=np.zeros((N, D)), scale=np.zeros((N, D)), mid=np.zeros((N, D)), ambiguous=np.zeros((N, D), bool),
               at_cut=np.zeros(N, bool))
    out["events"][:, D] = np.float32(dataset)
    took_bottom, took_top = np.zeros((N, D), bool), np.zeros((N, D), bool)
    active = np.arange(N, dtype=np.int64)
    for t in range(ATTEMPTS):
        if active.size == 0:
            break
        ta, tb = (t, t + 1) if variant == "single_counter" else (2 * t, 2 * t + 1)
        A = words(active, np.full(active.size, ta), seed)
        w = [A[1], A[2], A[3]]
        if D == 4:
            w.append(A[3] if variant == "reuse_word" else words(active, np.full(active.size, tb), seed)[0])
        pos = ((((A[1] if variant == "row_from_y" else A[0]) * np.uint64(n)) >> np.uint64(32)) & U32).astype(np.int64)
        i = row_index[pos]
        factor = lam[pos] if variant == "lam_by_position" else lam[i]
        ok = np.ones(active.size, bool)
        near_cut = fragile[pos].copy()
        x = np.zeros((active.size, D), np.float32)
        for k in range(D):
            xd, hw = point(rows_c[pos, k], factor, w[k], h[k], lower[k], upper[k], variant)
            bottom, top = ends[k]
            if variant == "clamp_before_round":
                xc = np.where(xd >= lower[k], xd, float(bottom))
                xf = np.where(xc < upper[k], xc, float(top)).astype(np.float32)
                tb_, tt_ = np.zeros(active.size, bool), np.zeros(active.size, bool)
            else:
                xf = xd.astype(np.float32)
                tb_ = ~(xf.astype(np.float64) >= lower[k])
                xf = np.where(tb_, bottom, xf)
                tt_ = ~(xf.astype(np.float64) < upper[k])
                xf = np.where(tt_, top, xf)
            scale = np.maximum(np.abs(xd), hw)
            mid = midpoint_distance(xd)
            delta = DELTA * scale
            amb = (mid <= delta) | (np.abs(xd - lower[k]) <= delta) | (np.abs(xd - upper[k]) <= delta)
            if has_cuts:
                ok &= ~((xf > cut_hi[k]) | (xf < cut_lo[k]))
                for c in (cut_lo[k], cut_hi[k]):
                    cd = float(c)
                    step = float(np.nextafter(np.float32(abs(cd)), np.float32(np.inf))) - abs(cd)
                    near_cut |= np.abs(xd - cd) <= delta
                    near_cut |= amb & (np.abs(xf.astype(np.float64) - cd) <= step)
            x[:, k] = xf
            out["xd"][active, k], out["scale"][active, k], out["mid"][active, k] = xd, scale, mid
            out["ambiguous"][active, k] = amb
            took_bottom[active, k], took_top[active, k] = tb_, tt_
        # an event keeps what its last attempt drew, as the kernel's registers do
        out["events"][active, :D] = x
        out["row"][active] = i
        out["attempts"][active] = t + 1
        out["at_cut"][active] |= near_cut
        active = active[~ok]
    out["exhausted"] = int(active.size)
    out["clamped_bottom"], out["clamped_top"] = int(took_bottom.sum()), int(took_top.sum())
    return out


def excused(d):
    """bool [n]: the events a comparison with the device may not hold to the bit."""
    return d["ambiguous"].any(axis=1) | d["at_cut"]


def changed_rows(a, b):
    """The share of events whose floats differ between two draws."""
    return float(np.mean(np.any(a["events"].view(np.uint32) != b["events"].view(np.uint32), axis=1)))


# ------------------------------------------------------------------------------------ the cases both test files run
SYSTS = [dict(type="shift", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
         dict(type="resolution_scale", obs=0, true_obs=2, pars=[2])]
PARAMS = {0: -0.35, 1: 0.06, 2: 0.25}
BIG_SEEDS = (7, 2 ** 32 + 7, 2 ** 63 + 12345)


class Case:
    """One evaluator and one call of RandomSample.  table float32 [N, nfields]; scale the bandwidth_scale; alpha the
    bandwidth sensitivity; cuts (lowers, uppers) or None."""

    def __init__(self, name, D, lower, upper, table, scale, nevents, seed, systs=(), params=None, alpha=0.0, cuts=None,
                 shared=False, dataset=0):
        self.name, self.D = name, D
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.table = np.ascontiguousarray(table, np.float32)
        self.nfields = self.table.shape[1]
        self.scale, self.nevents, self.seed = [float(v) for v in scale], int(nevents), int(seed)
        self.systs, self.params, self.alpha, self.cuts = list(systs), dict(params or {}), float(alpha), cuts
        self.shared, self.dataset = shared, dataset

    def replay(self, h, lam=None, variant=None):
        """draw() on this case, with the evaluator's bandwidths (and factors): (the draw, n in-domain rows)."""
        rows_c, idx, fragile = prepare(self.table, self.nfields, self.D, self.lower, self.upper, h, self.systs,
                                       self.params)
        lam = np.ones(len(self.table)) if lam is None else lam
        lo, hi = self.cuts if self.cuts else (None, None)
        return draw(rows_c, idx, lam, h, self.lower, self.upper, self.nevents, self.seed, lo, hi, self.dataset, variant,
                    fragile), len(idx)


def _dims_table(rng, D, N):
    """N rows of D observables in [0, 4) x [-1, 1) x [0, 6) x [-2, 3), about 10 % outside, interleaved."""
    lower, upper = np.array([0.0, -1.0, 0.0, -2.0])[:D], np.array([4.0, 1.0, 6.0, 3.0])[:D]
    mid, wid = (lower + upper) / 2, upper - lower
    x = mid + wid * np.clip(rng.normal(0.0, 0.22, (N, D)), -0.499, 0.499)
    out = rng.random(N) < 0.1
    x[out, rng.integers(0, D, int(out.sum()))] += wid[0] * 3
    return x.astype(np.float32), lower, upper


def dims_case(D, seed):
    x, lower, upper = _dims_table(np.random.default_rng(8100 + D), D, 1000)
    return Case("D%d_seed%d" % (D, BIG_SEEDS.index(seed)), D, lower, upper, x, [0.9, 1.1, 0.8, 1.2][:D], 100000, seed)


def compaction_case(N):
    """Every third row outside the domain; rows 0, 255, 256 and N - 1 inside."""
    rng = np.random.default_rng(8200 + N)
    x = rng.uniform(0.5, 9.5, N)
    outside = np.arange(N) % 3 == 1
    outside[[i for i in (0, 255, 256, N - 1) if i < N]] = False
    x[outside] = rng.uniform(10.5, 12.0, int(outside.sum()))
    return Case("compaction_%d" % N, 1, [0.0], [10.0], x.astype(np.float32)[:, None], [1.0], 50000, 31 + N)


def systematics_case():
    """Fields (e, r, e_true): a shift of r, a scale and a resolution scale of e, large enough that rows leave the domain
    and rows that start outside it enter."""
    rng = np.random.default_rng(8300)
    N = 2000
    t = rng.normal(2.0, 0.9, N)
    tab = np.stack([t + rng.normal(0, 0.3, N), rng.uniform(-1.3, 1.3, N), t], axis=1)
    return Case("systematics", 2, [0.0, -1.0], [4.0, 1.0], tab, [1.0, 0.8], 100000, 41, SYSTS, PARAMS)


def adaptive_case(shared=False):
    rng = np.random.default_rng(8400)
    N = 1500
    x = np.stack([np.where(rng.random(N) < 0.3, rng.normal(2.0, 0.1, N), rng.uniform(0.0, 4.0, N)),
                  rng.normal(0.0, 0.45, N)], axis=1)
    outside = np.arange(N) % 4 == 2
    x[outside, 0] = rng.uniform(4.2, 5.0, int(outside.sum()))
    return Case("adaptive_shared" if shared else "adaptive", 2, [0.0, -1.0], [4.0, 1.0], x, [1.0, 1.0], 100000, 51,
                alpha=0.5, shared=shared)


def extreme_case(scale, lo=0.1, hi=0.2, reach=2e-5):
    """[lo, hi), neither bound a float; samples within `reach` of either end."""
    rng = np.random.default_rng(8500)
    x = np.concatenate([lo + reach * rng.random(500), hi - reach * rng.random(500)]).astype(np.float32)
    rng.shuffle(x)
    name = "bandwidth_x%g" % scale + ("" if lo == 0.1 else "_from_%g" % lo)
    return Case(name, 1, [lo], [hi], x[:, None], [scale], 100000, 61, dataset=3)


def cuts_case():
    """Cuts that keep about 30 % of the mass."""
    x, lower, upper = _dims_table(np.random.default_rng(8600), 2, 1000)
    return Case("cuts", 2, lower, upper, x, [1.0, 1.0], 100000, 71, cuts=([1.5, -0.4], [3.0, 0.25]))


def exhaustion_case():
    """Cuts that keep about 0.5 %: some of the events pass no attempt."""
    rng = np.random.default_rng(8700)
    x = rng.normal(5.0, 1.5, 1000).astype(np.float32)
    return Case("exhaustion", 1, [0.0], [10.0], x[:, None], [1.0], 20000, 81, cuts=([7.5], [7.57]))


def stride_case():
    """More events than 4096 x 256 lanes: lanes take a second event."""
    rng = np.random.default_rng(8800)
    x = rng.uniform(-0.5, 10.5, 300).astype(np.float32)
    return Case("grid_stride", 1, [0.0], [10.0], x[:, None], [1.0], 1048576 + 257, 91)


COMPACTION_COUNTS = (255, 256, 257, 70001)


def cases():
    """Every case of tests/test_gpu_kde_sample_replay.py, by name."""
    out = [dims_case(D, seed) for D in (1, 2, 3, 4) for seed in BIG_SEEDS]
    out += [compaction_case(N) for N in COMPACTION_COUNTS]
    out += [systematics_case(), adaptive_case(), adaptive_case(shared=True), extreme_case(0.001), extreme_case(50.0),
            extreme_case(0.001, 0.7, 0.8), extreme_case(1e-6, reach=5e-8), cuts_case(), exhaustion_case(), stride_case()]
    return {c.name: c for c in out}


def check_replay(case, d, n):
    """What a case promises of its own replay (asserted by the CPU test with the host's bandwidths and by the GPU test
    with the evaluator's): the paths it is there to reach are reached."""
    picked = np.unique(d["row"]).size
    if case.name.startswith("compaction") and len(case.table) <= 257:
        assert picked == n, "%s: %d of %d in-domain rows picked" % (case.name, picked, n)
    if case.name == "compaction_70001":
        assert n > 2 * 16384                               # more than two scan blocks of in-domain rows
    if case.name == "bandwidth_x0.001":
        # float32(0.1) > 0.1: no float lies below a draw that is >= lower, so only the upper clamp can be taken here;
        # bandwidth_x0.001_from_0.7 (float32(0.7) < 0.7 and float32(0.8) > 0.8) takes both
        assert float(np.float32(0.1)) > 0.1 and float(np.float32(0.2)) > 0.2
        assert d["clamped_top"] > 0 and d["clamped_bottom"] == 0
        assert np.any(d["events"][:, 0] == end_floats(case.lower[0], case.upper[0])[0])
    if case.name == "bandwidth_x0.001_from_0.7":
        assert float(np.float32(0.7)) < 0.7 and d["clamped_top"] > 0 and d["clamped_bottom"] > 0
    if case.name == "bandwidth_x1e-06":
        assert d["clamped_top"] > 0.01 * case.nevents
    if case.name == "bandwidth_x50":
        assert np.all(d["scale"][:, 0] > 2 * (case.upper[0] - case.lower[0]))       # m is small
    if case.name == "cuts":
        assert d["attempts"].max() >= 8 and d["exhausted"] == 0
        assert 0.25 < np.mean(d["attempts"] == 1) < 0.35
    if case.name == "exhaustion":
        assert 0 < d["exhausted"] < case.nevents
    if case.name == "systematics":
        f0 = ref_transform(case.table, case.nfields, [], {})[:, :case.D]
        f1 = ref_transform(case.table, case.nfields, case.systs, case.params)[:, :case.D]
        lo, hi = np.asarray(case.lower), np.asarray(case.upper)
        in0, in1 = (np.all((f >= lo) & (f < hi), axis=1) for f in (f0, f1))
        assert (in0 & ~in1).sum() >= 20 and (~in0 & in1).sum() >= 20
    if case.name.startswith("adaptive"):
        x = case.table[:, :case.D].astype(np.float64)
        idx = np.flatnonzero(np.all((x >= np.asarray(case.lower)) & (x < np.asarray(case.upper)), axis=1))
        assert idx.size == n and np.mean(idx != np.arange(n)) > 0.9     # the place in the list is not the table row
    if case.name == "grid_stride":
        assert case.nevents > 4096 * 256


# ------------------------------------------------------------------------------------ replay-only controls
def tail_control():
    """A bandwidth ten million times the domain, about zero, where floats are dense: the one shape at which the rounding of
    1 - p moves events (every case of cases() gives the same floats either way).  Not for the device: delta is wider
    than the float spacing here, every event is ambiguous."""
    rng = np.random.default_rng(8900)
    x = rng.uniform(-1e-7, 1e-7, 300).astype(np.float32)
    c = Case("tail_control", 1, [-1e-7], [1e-7], x[:, None], [1.0], 50000, 95)
    return c, np.array([1.0])


# ------------------------------------------------------------------------------------ the law
def ks_distance(events, s, h, lo, hi):
    """sup |F_N - F| against the exact mixture CDF (tests/test_gpu_kde_sample.ks_distance)."""
    from tests.kde_reference import mixture_cdf
    grid = np.linspace(lo, hi, 4001)
    F = np.interp(np.sort(events), grid, mixture_cdf(grid, s, h, lo, hi))
    n = len(events)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)))


# ------------------------------------------------------------------------------------ the comparison
def float_steps(a, b):
    """How many floats apart two float32 arrays are (0: the same bits, but -0.0 and 0.0 one apart)."""
    def ordinal(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF) - 1, i)
    return np.abs(ordinal(a) - ordinal(b))


def compare(got, d, label=""):
    """Device events against a draw.  Every event that is not excused equal in all D + 1 floats as bytes; an event with
    ambiguous coordinates at most one float step off in those and equal in the others; an event ambiguous as a whole
    (at_cut) left out.  Prints the one-step mismatches, each with the replay's distance to the float midpoint in units of
    2^-53 max(|xd|, hw).  Returns dict(ok, wrong, one_step, largest, excused)."""
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape == d["events"].shape
    D = got.shape[1] - 1
    steps = float_steps(got, d["events"])
    allowed = np.zeros(steps.shape, np.int64)
    allowed[:, :D] = d["ambiguous"]
    allowed[d["at_cut"]] = np.iinfo(np.int64).max
    wrong = np.flatnonzero(np.any(steps > allowed, axis=1))
    ev, k = np.nonzero((steps[:, :D] == 1) & d["ambiguous"] & ~d["at_cut"][:, None])
    dist = d["mid"][ev, k] / (2.0 ** -53 * d["scale"][ev, k])
    share = float(np.mean(excused(d))) if len(got) else 0.0
    print("%s: %d events, %d wrong, %d one float off where ambiguous, %.3g of the events excused"
          % (label, len(got), wrong.size, ev.size, share))
    for e, kk, u in zip(ev, k, dist):
        print("  event %d observable %d: the replay's xd is %.1f x 2^-53 max(|xd|, hw) from the midpoint" % (e, kk, u))
    for e in wrong[:5]:
        print("  event %d: device %r, replay %r (row %d, attempts %d)" % (e, got[e], d["events"][e], d["row"][e],
                                                                       d["attempts"][e]))
    return dict(ok=wrong.size == 0 and share <= 1e-3, wrong=int(wrong.size), one_step=int(ev.size),
                largest=float(dist.max()) if dist.size else None, excused=share)


def host_bandwidths(case):
    """Scott's rule in numpy (tests/kde_reference.ref_bandwidths): what the CPU tests use where the GPU tests take
    ev.Bandwidths() (equal to 1e-12 relative: tests/test_gpu_kde_sample.py)."""
    from tests.kde_reference import ref_bandwidths
    return ref_bandwidths(case.table, case.nfields, case.D, np.asarray(case.lower), np.asarray(case.upper), case.scale)


def host_factors(case):
    """The local factors in numpy (tests/kde_adaptive_reference.ref_local_factors, equal to the device's to 1e-11), or
    ones."""
    if case.alpha == 0.0:
        return np.ones(len(case.table))
    from tests.kde_adaptive_reference import ref_local_factors
    return ref_local_factors(case.table, case.nfields, case.D, np.asarray(case.lower), np.asarray(case.upper),
                             case.scale, case.alpha)
