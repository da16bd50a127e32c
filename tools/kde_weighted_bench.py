"""Measures pdfz::EvalKernel over weighted Monte Carlo samples against the unweighted evaluator on the same table, in one
run, and prints one JSON line.

The shape of tools/kde_bench.py: N = 2^17 samples, D = 2 observables, nfields = 3, shift + scale + resolution
systematics, E = 10^5 evaluation points; multiplicities uniform in 0 ... 80.  The yardstick is the unweighted evaluator:
both are warmed, then measured alternately, --repeats times each (host clock around EvalAsync + EvalFinished over a
window of at least --seconds).  unweighted_spread is the relative spread between the yardstick's own repeats; the weighted
evaluation is expected inside it (the pair sum is the same machine code; the prepass, 0.6 % of an evaluation, reads 4
more bytes per row).  Alongside, each for both evaluators: ms_per_sample_call (RandomSample of --sample-events events,
median of 5 after one warm-up), ms_per_projection (Project onto --project-bins bins, both observables, mean over at least
half of --seconds) and ms_construct_adaptive (host clock around the adaptive construction, sensitivity 0.5, after one
warm-up construction).
Usage: python tools/kde_weighted_bench.py [--samples N] [--points E] [--seconds S] [--repeats R] [--sample-events M]
                                          [--project-bins B]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sxmc_amd import capi, pdfz  # noqa: E402
from sxmc_amd.capi import DeviceArray  # noqa: E402
from tools.kde_bench import eval_window  # noqa: E402


def built(samples, F, D, lower, upper, m, pts, par, alpha=0.0):
    ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D, bandwidth_sensitivity=alpha, multiplicities=m)
    ev.AddSystematic(pdfz.ShiftSystematic(1, [0]))
    ev.AddSystematic(pdfz.ScaleSystematic(0, [1]))
    ev.AddSystematic(pdfz.ResolutionScaleSystematic(0, 2, [2]))
    ev.SetEvalPoints(pts.ravel())
    pdf, norm = DeviceArray.zeros(pts.shape[0], np.float32), DeviceArray.zeros(1, np.uint32)
    ev.SetPDFValueBuffer(pdf)
    ev.SetNormalizationBuffer(norm)
    ev.SetParameterBuffer(par)
    return ev, pdf, norm


def sample_ms(ev, nevents):
    ev.RandomSample(nevents, 1)
    out = []
    for k in range(5):
        c0 = time.perf_counter()
        ev.RandomSample(nevents, 2 + k)
        out.append(1e3 * (time.perf_counter() - c0))
    return float(np.median(out))


def projection_ms(ev, D, nbins, seconds):
    for k in range(D):
        ev.Project(k, nbins)
    calls, t0 = 0, time.perf_counter()
    while True:
        for k in range(D):
            ev.Project(k, nbins)
        calls += D
        el = time.perf_counter() - t0
        if el >= seconds and calls >= 3 * D:
            return 1e3 * el / calls


def construct_ms(samples, F, D, lower, upper, m):
    sync = capi.load().sxmc_device_synchronize
    out = []
    for _ in range(2):                                   # (the first warms the pilot's code and the allocator)
        c0 = time.perf_counter()
        ev = pdfz.EvalKernel(samples.ravel(), F, D, lower, upper, [1.0] * D, bandwidth_sensitivity=0.5, multiplicities=m)
        sync()
        out.append(1e3 * (time.perf_counter() - c0))
        ev.close()
    return out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 17)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--sample-events", type=int, default=1000000)
    ap.add_argument("--project-bins", type=int, default=100)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("kde_weighted_bench.py needs a GPU")
    D, F = 2, 3
    rng = np.random.default_rng(11)
    n, e = a.samples, a.points
    t = rng.normal(5.0, 1.5, n)
    samples = np.stack([t + rng.normal(0, 0.4, n), rng.uniform(-1, 1, n), t], axis=1).astype(np.float32)
    lower, upper = [0.0, -1.0], [10.0, 1.0]
    pts = np.stack([rng.uniform(0, 10, e), rng.uniform(-1, 1, e), np.zeros(e)], axis=1).astype(np.float32)
    m = rng.integers(0, 81, n).astype(np.uint32)
    par = DeviceArray(np.array([0.01, 0.02, 0.05]))
    plain, _, norm_p = built(samples, F, D, lower, upper, None, pts, par)
    weighted, pdf_w, norm_w = built(samples, F, D, lower, upper, m, pts, par)
    for ev in (plain, weighted):                         # warm both
        eval_window(ev, 0.2)
    ms = {"unweighted": [], "weighted": []}
    for _ in range(max(a.repeats, 1)):                   # alternate them
        ms["unweighted"].append(eval_window(plain, a.seconds)[0])
        ms["weighted"].append(eval_window(weighted, a.seconds)[0])
    up, wp = float(np.mean(ms["unweighted"])), float(np.mean(ms["weighted"]))
    spread = (max(ms["unweighted"]) - min(ms["unweighted"])) / up
    out = dict(tool="kde_weighted_bench", samples=n, points=e, observables=D, multiplicities="uniform 0..80",
               ms_per_eval_unweighted=[round(v, 4) for v in ms["unweighted"]],
               ms_per_eval_weighted=[round(v, 4) for v in ms["weighted"]],
               weighted_over_unweighted=round(wp / up, 5), unweighted_spread=round(spread, 5),
               norm_unweighted=int(norm_p.get()[0]), norm_weighted=int(norm_w.get()[0]),
               n_eff=weighted.EffectiveSamples(), finite_values_weighted=int(np.isfinite(pdf_w.get()).sum()),
               sample_events=a.sample_events,
               ms_per_sample_call_unweighted=round(sample_ms(plain, a.sample_events), 4),
               ms_per_sample_call_weighted=round(sample_ms(weighted, a.sample_events), 4),
               project_bins=a.project_bins,
               ms_per_projection_unweighted=round(projection_ms(plain, D, a.project_bins, a.seconds / 2), 4),
               ms_per_projection_weighted=round(projection_ms(weighted, D, a.project_bins, a.seconds / 2), 4))
    plain.close()
    weighted.close()
    out["ms_construct_adaptive_unweighted"] = round(construct_ms(samples, F, D, lower, upper, None), 3)
    out["ms_construct_adaptive_weighted"] = round(construct_ms(samples, F, D, lower, upper, m), 3)
    out["device"] = capi.device_info(0)["name"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
