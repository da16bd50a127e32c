"""Measures pdfz::EvalKernel, the kernel-density PDF, and prints one JSON line.

Default shape: N = 2^17 samples, D = 2 observables, nfields = 3 (the third a true value), shift + scale + resolution
systematics, E = 10^5 evaluation points.  ms_per_eval: host clock around EvalAsync + EvalFinished (which waits for
the device), warmed up, over a window of at least --seconds.  pairs_per_s = E x N / that time.

The bound is the pair kernel's vector issue, read from its inner loop (kde_kernels.hip, --save-temps ISA): per sample
and wave, D v_sub_f32, one v_mul_f32, D - 1 v_fmac_f32 for the distance, one v_exp_f32 and one v_fmac_f32 to
accumulate; the sample row comes through scalar loads as SGPR operands.  At the issue costs of one wave's stream
(4 cycles, 8 for v_exp_f32) that is 4 (2D + 1) + 8 cycles per 64 pairs per SIMD (28 at D = 2), over 4 SIMDs per CU at
the clock the device reports.  cpu_numpy_pairs_per_s: the same sum in numpy f64 on a subset of the points.
ms_per_sample_call: host clock around RandomSample(--sample-events) from the last evaluation (compaction of the
in-domain rows, the draw, the copy of the events to the host), median of 5 calls after one warm-up.
ms_per_projection: host clock around one Project(obs, --project-bins) of the last evaluation (the per-row scratch, the
sum over samples x bins, the combine, the copy of the shares to the host), both observables in turn, mean per call over
a window of at least half of --seconds after one warm-up each.
--adaptive: besides, in the same run, an evaluator with adaptive bandwidths (--sensitivity, default 0.5) on the same
table, systematics and points: ms_per_eval_adaptive measured the same way right after the fixed-bandwidth window,
adaptive_over_fixed their ratio (expected from the instruction count alone: one more v_mul_f32, 32 cycles per 64 pairs
against 28, 1.14), and ms_pilot, the host clock around the adaptive construction minus that around a fixed-bandwidth
construction of the same table made just before (both in the line): what the pilot, the factors and their upload add.
--cv: instead of all the above, bandwidth cross-validation on the same table (one JSON line, tool "kde_bench_cv"):
ms_pilot as above (the yardstick, in the same run); ms_scan, the host clock around one CvScores call of the default
grid's K = 21 candidates on every in-domain row (rows read back, constants and weights, the fused pair kernel, the
logarithms back and added); scan_over_k_pilots = ms_scan / (21 ms_pilot), and the same per pair (the pilot takes every
table row against the in-domain rows, a scan the in-domain rows against themselves); ms_search_all_rows and
ms_search_default, the host clock around SelectBandwidthScale with max_rows = 0 and with the default max_rows, and what
they chose.
--cutoff: instead of all the above, the cutoff radius (EvalKernel.SetCutoff) at the default shape, fixed and adaptive
bandwidths in one process (one JSON line, tool "kde_bench_cutoff"): per R in 0, 0 again (the run-to-run spread), +inf
(every pair, in sorted order: the price of the gather and the mask walk), 6 and 4 the ms per evaluation measured as
above, tiles_visited / tiles_possible of the last evaluation, and the largest relative change of a value against
R = 0; and the host clock around SetEvalPoints without and with the point-side sort.
Usage: python tools/kde_bench.py [--samples N] [--points E] [--seconds S] [--cpu-points K] [--sample-events M]
                                 [--project-bins B] [--adaptive] [--sensitivity A] [--cv] [--cutoff]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sxmc_amd import capi, pdfz  # noqa: E402
from sxmc_amd.capi import DeviceArray  # noqa: E402


def eval_window(ev, seconds):
    """(ms per EvalAsync + EvalFinished, calls): three warm-up evaluations, then a window of at least `seconds`."""
    for _ in range(3):
        ev.EvalAsync()
        ev.EvalFinished()
    calls, t0 = 0, time.perf_counter()
    while True:
        ev.EvalAsync()
        ev.EvalFinished()
        calls += 1
        el = time.perf_counter() - t0
        if el >= seconds and calls >= 3:
            return 1e3 * el / calls, calls


def measure_adaptive(a, samples, F, D, lower, upper, pts, par, fixed_ms):
    """The --adaptive keys of the result line."""
    e = pts.shape[0]
    c0 = time.perf_counter()
    plain = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0, 1.0])
    capi.load().sxmc_device_synchronize()
    c1 = time.perf_counter()
    ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0, 1.0], bandwidth_sensitivity=a.sensitivity)
    capi.load().sxmc_device_synchronize()
    c2 = time.perf_counter()
    plain.close()
    ev.AddSystematic(pdfz.ShiftSystematic(1, [0]))
    ev.AddSystematic(pdfz.ScaleSystematic(0, [1]))
    ev.AddSystematic(pdfz.ResolutionScaleSystematic(0, 2, [2]))
    ev.SetEvalPoints(pts.ravel())
    pdf, norm = DeviceArray.zeros(e, np.float32), DeviceArray.zeros(1, np.uint32)
    ev.SetPDFValueBuffer(pdf)
    ev.SetNormalizationBuffer(norm)
    ev.SetParameterBuffer(par)
    ms, calls = eval_window(ev, a.seconds)
    lam = ev.LocalFactors()
    out = dict(sensitivity=a.sensitivity, ms_per_eval_adaptive=round(ms, 4), evaluations_adaptive=calls,
               adaptive_over_fixed=round(ms / fixed_ms, 4), expected_adaptive_over_fixed=round(32 / 28, 4),
               ms_construct_fixed=round(1e3 * (c1 - c0), 3), ms_construct_adaptive=round(1e3 * (c2 - c1), 3),
               ms_pilot=round(1e3 * ((c2 - c1) - (c1 - c0)), 3), factor_min=float(lam.min()),
               factor_max=float(lam.max()), factors_clipped=int(np.sum((lam == 0.1) | (lam == 10.0))),
               norm_adaptive=int(norm.get()[0]), finite_values_adaptive=int(np.isfinite(pdf.get()).sum()))
    ev.close()
    return out


def measure_cv(a, samples, F, D, lower, upper):
    """The result line of --cv."""
    sync = capi.load().sxmc_device_synchronize
    pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D, bandwidth_sensitivity=a.sensitivity).close()   # warm
    c0 = time.perf_counter()
    ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D)
    sync()
    c1 = time.perf_counter()
    ad = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D, bandwidth_sensitivity=a.sensitivity)
    sync()
    c2 = time.perf_counter()
    ad.close()
    ms_pilot = 1e3 * ((c2 - c1) - (c1 - c0))
    o = pdfz.CvOptions()
    grid = o.lo * (o.hi / o.lo) ** (np.arange(o.steps) / (o.steps - 1))
    cand = grid[:, None] * ev.Bandwidths()[None, :]           # (the multipliers on the evaluator's own Scott bandwidths)
    ev.CvScores(cand, 4096)                                   # warm: the kernels' code, the allocator
    t0 = time.perf_counter()
    scores, m = ev.CvScores(cand, 0)
    ms_scan = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    full = ev.SelectBandwidthScale(pdfz.CvOptions(max_rows=0))
    ms_full = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    dflt = ev.SelectBandwidthScale(o)
    ms_default = 1e3 * (time.perf_counter() - t0)
    n = samples.shape[0]
    pilot_pairs, scan_pairs = float(n) * m, float(m) * m
    ev.close()
    return dict(tool="kde_bench_cv", samples=n, observables=D, rows_scored=int(m), candidates=int(o.steps),
                ms_construct_fixed=round(1e3 * (c1 - c0), 3), ms_construct_adaptive=round(1e3 * (c2 - c1), 3),
                ms_pilot=round(ms_pilot, 3), ms_scan=round(ms_scan, 3),
                scan_over_k_pilots=round(ms_scan / (o.steps * ms_pilot), 4),
                scan_over_k_pilots_per_pair=round((ms_scan / scan_pairs) / (o.steps * ms_pilot / pilot_pairs), 4),
                finite_scores=int(np.isfinite(scores).sum()), best_multiplier_of_scan=float(grid[int(np.nanargmax(scores))]),
                ms_search_all_rows=round(ms_full, 3), chosen_all_rows=[float(v) for v in full.scale],
                score_all_rows=full.score, score_at_one_all_rows=full.score_at_one,
                ms_search_default=round(ms_default, 3), rows_default=dflt.rows_used,
                chosen_default=[float(v) for v in dflt.scale], at_edge_default=dflt.at_edge,
                device=capi.device_info(0)["name"])


def measure_cutoff(a, samples, F, D, lower, upper, pts, params):
    """The result line of --cutoff: fixed and adaptive, ms per evaluation at R = 0 (twice: the run-to-run spread),
    +inf (the price of the gather and the mask walk), 6 and 4, with the visited share of the tiles and the largest
    relative change of a value against R = 0 over the values above 1e-3 of the largest."""
    e = pts.shape[0]
    par = DeviceArray(params)
    out = dict(tool="kde_bench_cutoff", samples=samples.shape[0], points=e, observables=D,
               systematics=["shift", "scale", "resolution_scale"], device=capi.device_info(0)["name"])
    for mode, alpha in (("fixed", 0.0), ("adaptive", a.sensitivity)):
        ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D, bandwidth_sensitivity=alpha)
        ev.AddSystematic(pdfz.ShiftSystematic(1, [0]))
        ev.AddSystematic(pdfz.ScaleSystematic(0, [1]))
        ev.AddSystematic(pdfz.ResolutionScaleSystematic(0, 2, [2]))
        c0 = time.perf_counter()
        ev.SetEvalPoints(pts.ravel())
        ms_points_plain = 1e3 * (time.perf_counter() - c0)
        pdf, norm = DeviceArray.zeros(e, np.float32), DeviceArray.zeros(1, np.uint32)
        ev.SetPDFValueBuffer(pdf)
        ev.SetNormalizationBuffer(norm)
        ev.SetParameterBuffer(par)
        rows, base = [], None
        for label, R in (("0", 0.0), ("0_again", 0.0), ("inf", math.inf), ("6", 6.0), ("4", 4.0)):
            c0 = time.perf_counter()
            ev.SetCutoff(R)
            ms_set = 1e3 * (time.perf_counter() - c0)
            ms, calls = eval_window(ev, a.seconds)
            visited, possible = ev.CutoffStats()
            v = pdf.get().astype(np.float64)
            if base is None:
                base = v
            big = base >= 1e-3 * np.nanmax(base)
            rows.append(dict(R=label, ms_per_eval=round(ms, 4), evaluations=calls, ms_set_cutoff=round(ms_set, 3),
                             tiles_visited=visited, tiles_possible=possible,
                             visited_fraction=round(visited / possible, 5) if possible else None,
                             worst_relative_change=float(np.max(np.abs(v[big] - base[big]) / base[big])),
                             norm=int(norm.get()[0])))
        c0 = time.perf_counter()
        ev.SetEvalPoints(pts.ravel())
        out[mode] = dict(rows=rows, ms_set_eval_points_plain=round(ms_points_plain, 3),
                         ms_set_eval_points_sorted=round(1e3 * (time.perf_counter() - c0), 3))
        ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 17)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--cpu-points", type=int, default=200)
    ap.add_argument("--sample-events", type=int, default=1000000)
    ap.add_argument("--project-bins", type=int, default=100)
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--sensitivity", type=float, default=0.5)
    ap.add_argument("--cv", action="store_true")
    ap.add_argument("--cutoff", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("kde_bench.py needs a GPU")
    D, F = 2, 3
    rng = np.random.default_rng(11)
    n, e = a.samples, a.points
    t = rng.normal(5.0, 1.5, n)
    samples = np.stack([t + rng.normal(0, 0.4, n), rng.uniform(-1, 1, n), t], axis=1).astype(np.float32)
    lower, upper = [0.0, -1.0], [10.0, 1.0]
    if a.cv:
        print(json.dumps(measure_cv(a, samples, F, D, lower, upper)))
        return
    if a.cutoff:
        pts = np.stack([rng.uniform(0, 10, e), rng.uniform(-1, 1, e), np.zeros(e)], axis=1).astype(np.float32)
        print(json.dumps(measure_cutoff(a, samples, F, D, lower, upper, pts, np.array([0.01, 0.02, 0.05]))))
        return
    ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0, 1.0])
    ev.AddSystematic(pdfz.ShiftSystematic(1, [0]))
    ev.AddSystematic(pdfz.ScaleSystematic(0, [1]))
    ev.AddSystematic(pdfz.ResolutionScaleSystematic(0, 2, [2]))
    pts = np.stack([rng.uniform(0, 10, e), rng.uniform(-1, 1, e), np.zeros(e)], axis=1).astype(np.float32)
    ev.SetEvalPoints(pts.ravel())
    params = np.array([0.01, 0.02, 0.05])
    pdf, norm, par = DeviceArray.zeros(e, np.float32), DeviceArray.zeros(1, np.uint32), DeviceArray(params)
    ev.SetPDFValueBuffer(pdf)
    ev.SetNormalizationBuffer(norm)
    ev.SetParameterBuffer(par)
    ms, calls = eval_window(ev, a.seconds)
    adaptive = measure_adaptive(a, samples, F, D, lower, upper, pts, par, ms) if a.adaptive else {}
    pairs = float(e) * n
    rate = pairs / (ms * 1e-3)
    info = capi.device_info(0)
    cycles = 4 * (2 * D + 1) + 8
    bound = info["compute_units"] * 4 * info["clock_khz"] * 1e3 * 64.0 / cycles
    values = pdf.get()

    # fake data: --sample-events events drawn from the last evaluation
    ev.RandomSample(a.sample_events, 1)
    sample_ms = []
    for k in range(5):
        c0 = time.perf_counter()
        drawn = ev.RandomSample(a.sample_events, 2 + k)
        sample_ms.append(1e3 * (time.perf_counter() - c0))
    sample_ms = float(np.median(sample_ms))
    drawn_in_domain = bool(np.all((drawn[:, :D] >= lower) & (drawn[:, :D] < upper)))

    # the projections of the last evaluation onto both observables
    shares = [ev.Project(k, a.project_bins) for k in range(D)]
    pcalls, p0 = 0, time.perf_counter()
    while True:
        for k in range(D):
            shares[k] = ev.Project(k, a.project_bins)
        pcalls += D
        pel = time.perf_counter() - p0
        if pel >= a.seconds / 2 and pcalls >= 3 * D:
            break
    projection_ms = 1e3 * pel / pcalls
    projection_sums = [float(m.sum()) for m in shares]

    # numpy f64 on a subset of the points (the bandwidths as the evaluator fixed them, parameters applied)
    h = ev.Bandwidths()
    x = samples.astype(np.float64)
    x[:, 1] = x[:, 1] + params[0]
    x[:, 0] = x[:, 0] * (1 + params[1])
    x[:, 0] = x[:, 0] + params[2] * (x[:, 0] - x[:, 2])
    s = x[:, :D]
    s = s[np.all((s >= lower) & (s < upper), axis=1)]
    k = min(a.cpu_points, e)
    sub = pts[:k, :D].astype(np.float64)
    c0 = time.perf_counter()
    for i in range(k):
        z = (sub[i] - s) / h
        np.exp(-0.5 * (z * z).sum(axis=1)).sum()
    cpu_rate = k * float(n) / (time.perf_counter() - c0)

    print(json.dumps(dict(tool="kde_bench", samples=n, points=e, observables=D, nfields=F,
                          systematics=["shift", "scale", "resolution_scale"], evaluations=calls,
                          ms_per_eval=round(ms, 4), pairs_per_s=rate, bound_pairs_per_s=bound,
                          bound_cycles_per_64_pairs_per_simd=cycles, clock_mhz=info["clock_khz"] / 1e3,
                          compute_units=info["compute_units"], fraction_of_bound=round(rate / bound, 4),
                          cpu_numpy_pairs_per_s=cpu_rate, norm=int(norm.get()[0]),
                          finite_values=int(np.isfinite(values).sum()), sample_events=a.sample_events,
                          ms_per_sample_call=round(sample_ms, 4), sampled_in_domain=drawn_in_domain,
                          project_bins=a.project_bins, ms_per_projection=round(projection_ms, 4),
                          projection_sums=projection_sums,
                          device=info["name"], **adaptive)))


if __name__ == "__main__":
    main()
