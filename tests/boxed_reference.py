"""The BOXED fill's decision, restated in numpy (fill_boxed_body, sxmc_amd/csrc/fill_kernels.inc.h; layout_kernels.hip).

fill_boxed_kernel counts a row without looking at its float values in two places, and "bit-exact" rests there on an
argument, not on an identity:
  * the STREAMED observable is binned from one 16-bit code per row when fract(u') >= thr (the boxed copy of THE BOUND,
    one field: NQ = 1); every other row goes to the exact queue;
  * the BOXED observable is one constant per 256-row granule when the reference's operations, run on the corners of the
    granule's box [xmin, xmax] x [tmin, tmax] (apply_box_interval, granule_meta), put both ends in one bin.
This module restates both, operation by operation -- IEEE double where the kernel uses double, float32 where it uses
float -- with the measurement build's two scales on the bound as keywords, and with PLANTED WRONG VARIANTS of the interval
rule, selectable by name: tests/test_boxed_model_cpu.py holds the restatement against the reference's per-row arithmetic
and shows that each variant, and a halved threshold, fail on the rows tests/boxed_rows.py builds.  No GPU here."""
import numpy as np

from tests.test_codes_model_cpu import fma32, reference_bins, windows   # noqa: F401  (shared with the ordered form's model)

QCODE_MAX = 65533
QCODE_EXACT = 0xFFFE        # outside the window, or failing the half-step check: "ask the exact columns"
QCODE_NEVER = 0xFFFF        # not finite: never counted
SKIP, ONE_BIN, MIXED = 0, 1, 2
E_ABOVE = 0x7FFFFFFF
VARIANTS = ("no_swap_negative_scale", "no_swap_negative_resolution", "matching_corners", "domain_on_index",
            "resolution_before_scale")


# ---------------------------------------------------------------------------------------------------- the codes
def encode16(col, base, step):
    """column_codes16_kernel: one 16-bit code per row of ONE column, window [base, base + 65534 step]."""
    x = np.asarray(col).astype(np.float64)
    fin = np.abs(x) < np.inf
    with np.errstate(all="ignore"):
        t = (x - base) / step
        exact = ~((t >= 0.0) & (t < QCODE_MAX + 1.0))
        q = np.where(exact | ~fin, 0.0, t).astype(np.int64)
        centre = base + (q.astype(np.float64) + 0.5) * step
        exact |= ~(np.abs(x - centre) <= 0.5 * step * (1.0 + 2.0 ** -20))
    return np.where(~fin, QCODE_NEVER, np.where(exact, QCODE_EXACT, q)).astype(np.int64)


def dbg_scale(s):
    """A scale as sxmc_group_set_debug_mode carries it (8 bits: 1 + 64 s): (the field's value, the scale it means)."""
    f = 1 + int(round(64 * s))
    return f, (f - 1) / 64.0


def streamed_bound(systs, params, obs, base, step, lo, hi, nb, rounding_scale=1.0, total_scale=1.0):
    """fill_boxed_body's block "the streamed observable's program composed into single precision over its code":
    apply_affine with NQ = 1 over the systematics that write observable `obs`, then alpha, g, mu, epsq, eps, the
    eps < 0.125 switch, e = 1.01 eps, slack = 2^-23 and af, gf, thr.  rounding_scale / total_scale: dbg bits 8-15 /
    16-23 of the measurement build (everything but Q / the whole threshold).  Returns a dict; ok False: no codes."""
    a, c = 1.0, 0.0
    mag = max(abs(base), abs(base + 65534.0 * step))
    wild = False
    with np.errstate(all="ignore"):
        for s in systs:
            raw = float(params[s["pars"][0]])
            wild = wild or not abs(raw) < np.inf            # (any coefficient of the program, as the kernel's `wild`)
            if s["obs"] != obs:
                continue
            p = 0.0 + raw * 1.0
            ap = abs(p)
            if s["type"] == "shift":
                c = c + p
                mag = mag + ap
            elif s["type"] == "scale":
                sc1 = 1 + p
                a = a * sc1
                c = c * sc1
                mag = mag * (1 + ap)
            elif s["type"] == "ctscale":
                sc1 = 1 + p
                a = a * sc1
                c = 1 + (c - 1) * sc1
                mag = 1 + (mag + 1) * (1 + ap)
            else:
                raise ValueError("the streamed observable of a boxed program reads no other field")
        sc = nb / (hi - lo)
        alpha = a * step * sc
        sum_abs = abs(alpha)
        g = c - lo
        g = g + a * (base + 0.5 * step)
        g = g * sc
        mu = sum_abs * 65536.0 + abs(g) + float(nb) + 0.25
        epsq = 0.5 * sum_abs * (1.0 + 2.0 ** -19)
        eps = epsq + mu * 2.0 ** -21 + (mag + abs(lo)) * sc * 2.0 ** -44
        ok = bool(eps < 0.125) and not wild
        e, slack = eps * 1.01, 2.0 ** -23
        if rounding_scale != 1.0 or total_scale != 1.0:
            e = (epsq + rounding_scale * (e - epsq)) * total_scale
            slack = slack * rounding_scale * total_scale
        return dict(ok=ok, af=np.float32(alpha), gf=np.float32(g + e), thr=np.float32(2.0 * e + slack), nb=int(nb),
                    alpha=alpha, g=g, e=e, eps=eps, Q=epsq, S=mu * 2.0 ** -21, D=(mag + abs(lo)) * sc * 2.0 ** -44)


def classify_codes(codes, bound):
    """coarse_unit, per row: (index, trusted, inside the domain, queued).  u' = fma(af, code, gf) in float32 -- a 24-bit
    times a 16-bit number is exact in double, so the product and the sum are formed there and rounded once --, fract with
    v_fract_f32's clamp, floor, and the clamp to the guard rows (index -1 or nbins: counted nowhere).  queued: the row
    goes to the exact queue (ambiguous, or its code says "ask the exact columns"); a "never counted" code is neither
    trusted nor queued."""
    codes = np.asarray(codes, np.int64)
    special = codes >= QCODE_EXACT
    never = codes >= QCODE_NEVER
    n = codes.shape[0]
    u = fma32(np.full(n, bound["af"], np.float32), codes.astype(np.float32), np.full(n, bound["gf"], np.float32))
    with np.errstate(all="ignore"):
        fl = np.floor(u)
        fr = np.minimum((u - fl).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
        amb = ~(fr >= bound["thr"])
        idx = np.clip(np.where(np.isfinite(fl), fl, -1.0), -1.0, float(bound["nb"])).astype(np.int64)
    trusted = ~amb & ~special
    inside = (idx >= 0) & (idx < bound["nb"])
    queued = (amb | special) & ~never
    return idx, trusted, inside, queued


# ------------------------------------------------------------------------------------------- the interval rule
def _fin(*xs):
    ok = np.ones(np.shape(xs[0]), bool)
    for x in xs:
        ok &= np.abs(x) < np.inf
    return ok


def box_interval(boxes, systs, params, obs, truth, variant=None):
    """run_box_interval: the systematics that write observable `obs`, on the box's corners.  boxes: (G, 4) float32
    {xmin, xmax, tmin, tmax}.  Returns (xl, xh, fin) in double.  variant: one of VARIANTS (a planted mistake)."""
    assert variant is None or variant in VARIANTS, variant
    b = np.asarray(boxes, np.float32).astype(np.float64)
    xl, xh, tl, th = b[:, 0].copy(), b[:, 1].copy(), b[:, 2], b[:, 3]
    xl0, xh0 = xl.copy(), xh.copy()
    with np.errstate(all="ignore"):
        fin = _fin(xl, xh, tl, th)
        for s in systs:
            if s["obs"] != obs:
                continue
            pc = 0.0 + float(params[s["pars"][0]]) * 1.0
            if s["type"] == "shift":
                xl = xl + pc
                xh = xh + pc
            elif s["type"] in ("scale", "ctscale"):
                sc1 = 1 + pc
                if s["type"] == "scale":
                    a, c = xl * sc1, xh * sc1
                else:
                    a, c = 1 + (xl - 1) * sc1, 1 + (xh - 1) * sc1
                swap = not sc1 >= 0.0 and variant != "no_swap_negative_scale"
                xl, xh = (c, a) if swap else (a, c)
            else:
                assert s["true_obs"] == truth, "the boxed observable reads one truth field"
                if variant == "matching_corners":
                    dl, dh = xl - tl, xh - th
                elif variant == "resolution_before_scale":
                    dl, dh = xl0 - th, xh0 - tl
                else:
                    dl, dh = xl - th, xh - tl                     # x - t, smallest and largest
                a, c = pc * dl, pc * dh
                swap = not pc >= 0.0 and variant != "no_swap_negative_resolution"
                ml, mh = (c, a) if swap else (a, c)
                fin &= _fin(dl, dh, ml, mh)
                xl = xl + ml
                xh = xh + mh
            fin &= _fin(xl, xh)
    return xl, xh, fin


def granule_verdict(boxes, systs, params, obs, truth, lo, hi, nb, use_q=True, variant=None):
    """granule_meta: (verdict per granule -- SKIP, ONE_BIN or MIXED --, the bin of a ONE_BIN granule).  (`canon`, the
    test that the granule's flat index stays below 2^22 and in its row of the LDS copy, only ever turns ONE_BIN into
    MIXED and is not restated.)"""
    xl, xh, fin = box_interval(boxes, systs, params, obs, truth, variant)
    with np.errstate(all="ignore"):
        osc = nb / (hi - lo)
        big = 2.0 ** 31
        i0 = np.trunc(np.clip(np.where(np.isnan(xl), 0.0, (xl - lo) * osc), -big, big)).astype(np.int64)
        i1 = np.trunc(np.clip(np.where(np.isnan(xh), 0.0, (xh - lo) * osc), -big, big)).astype(np.int64)
        if variant == "domain_on_index":
            e0 = np.where(i0 < 0, -1, np.where(i0 >= nb, E_ABOVE, i0))
            e1 = np.where(i1 < 0, -1, np.where(i1 >= nb, E_ABOVE, i1))
        else:
            e0 = np.where(~(xl >= lo), -1, np.where(~(xl < hi), E_ABOVE, i0))
            e1 = np.where(~(xh >= lo), -1, np.where(~(xh < hi), E_ABOVE, i1))
    same = fin & (e0 == e1)
    skip = same & ((e0 < 0) | (e0 == E_ABOVE))
    mixed = ~same | (not use_q)
    verdict = np.where(skip, SKIP, np.where(mixed, MIXED, ONE_BIN))
    return verdict, e0


# ------------------------------------------------------------------------------------------------- the layout
def _ordered_bits(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u >> 31 != 0, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def layout_granules(tab, obs, truth, unwritten, lo, hi, nb, nstrata=2):
    """How the boxed table's rows fall into granules (get_bucket_sort, box_key_kernel, bucket_granules): buckets by the
    bins of the observables nothing writes; inside a bucket rows sorted (stably) by (stratum of x - t, x without its
    last four bits), the strata's bounds quantiles of x - t over the table; cut into 256 rows, each bucket padded.
    Returns (list of row-index arrays, boxes (G, 4) float32).  Rows outside the unwritten observables' domains are left
    out, as the table leaves them out.  The tests' claims hold for ANY grouping; this one is the library's."""
    tab = np.asarray(tab, np.float32)
    n = tab.shape[0]
    x, t = tab[:, obs], tab[:, truth]
    d = (x - t).astype(np.float32)
    kd = np.where(np.isnan(d), np.uint64(0xFFFFFFFF), _ordered_bits(d))
    stratum = np.zeros(n, np.uint64)
    if nstrata > 1:
        srt = np.sort(kd, kind="stable")
        for k in range(nstrata - 1):
            stratum += (srt[int(float(n) * (k + 1) / nstrata)] <= kd).astype(np.uint64)
    key = np.where(np.isnan(d) | np.isnan(x), np.uint64(0xFFFFFFFF), (stratum << np.uint64(28)) | (_ordered_bits(x) >> np.uint64(4)))
    bucket = np.zeros(n, np.int64)
    kept = np.ones(n, bool)
    for k in unwritten:
        v = tab[:, k].astype(np.float64)
        with np.errstate(all="ignore"):
            kept &= (v >= lo[k]) & (v < hi[k])
            i = np.where(kept, (v - lo[k]) * (nb[k] / (hi[k] - lo[k])), 0.0).astype(np.int64)
        bucket = bucket * (nb[k] + 1) + i
    rows = np.flatnonzero(kept)
    rows = rows[np.argsort(key[rows], kind="stable")]
    rows = rows[np.argsort(bucket[rows], kind="stable")]
    groups, boxes = [], []
    bsorted = bucket[rows]
    starts = np.flatnonzero(np.r_[True, bsorted[1:] != bsorted[:-1]])
    ends = np.r_[starts[1:], rows.size]
    for s0, s1 in zip(starts, ends):
        for at in range(int(s0), int(s1), 256):
            g = rows[at:min(at + 256, int(s1))]
            groups.append(g)
            xs, ts = x[g], t[g]
            if np.all(np.isfinite(xs)) and np.all(np.isfinite(ts)):
                boxes.append([xs.min(), xs.max(), ts.min(), ts.max()])
            else:
                boxes.append([np.nan] * 4)
    return groups, np.asarray(boxes, np.float32).reshape(-1, 4)


def decided_row_share(tab, groups, boxes, systs, params, obs, truth, lo, hi, nb):
    """The share of the table's in-domain rows (the reference's) that sit in granules the interval rule decides without
    the float path -- what a fill that drops its queues (measurement hook 16) still counts, when the streamed
    observable never decides."""
    verdict, _ = granule_verdict(boxes, systs, params, obs, truth, lo[obs], hi[obs], nb[obs])
    _, ind, _ = reference_bins(tab, systs, params, lo, hi, nb)
    decided = np.zeros(np.asarray(tab).shape[0], bool)
    for g in np.flatnonzero(verdict != MIXED):
        decided[groups[g]] = True
    return float((decided & ind).sum()) / float(ind.sum())
