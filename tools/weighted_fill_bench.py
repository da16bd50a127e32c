"""Measures the weighted histogram fill (sample multiplicities, include/sxmc_hip.h) against its yardstick and prints one
JSON line.

Shape: BASELINE config 3 (12 signals, 1e8 rows in all, 3 observables + a truth field, 20^3 bins, shift + scale +
resolution scale; --scale shrinks the row counts).  Two groups over tables of the same rows:
  weighted    every row with a uniform random multiplicity of mean 40 (0 ... 80): the weighted fill, 20 bytes per row;
  rows        the same tables unweighted in the ROWS form -- bucketing, ordering and pre-binning off --, 16 bytes per row:
              the yardstick, measured beside the weighted fill in the same run.
Fill time per evaluation: the dispatches' own begin and end timestamps (sxmc_group_profile), summed over the launches of
an evaluation, mean over --evals evaluations after --warmup; the two groups alternate, --repeats times (default 2).
Reported: every repeat's two times, their ratio, the spread between the repeats, and each fill's share of the 8 TB/s HBM
peak from the bytes it must stream (sxmc_group_algorithmic_bytes: tables and multiplicities).
Usage: python tools/weighted_fill_bench.py [--scale S] [--evals N] [--warmup W] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sxmc_amd import capi, nll, pdfz, workloads  # noqa: E402
from sxmc_amd.capi import DeviceArray  # noqa: E402
from sxmc_amd.mcmc import make_systematic  # noqa: E402

HBM_PEAK = 8.0e12


def build(w, mult, params, stream):
    evs = []
    norms = DeviceArray.zeros(w.nsignals, np.uint32)
    for j, s in enumerate(w.signals):
        ev = pdfz.EvalHist(s.samples, s.nfields, w.nobs, w.lower, w.upper, w.nbins, dataset=s.dataset)
        for d in w.systematics:
            ev.AddSystematic(make_systematic(d))
        if mult is not None:
            ev.SetSampleMultiplicities(mult[j])
        ev.SetNormalizationBuffer(norms, j)
        ev.SetParameterBuffer(params, w.nsources)
        evs.append(ev)
    g = nll.EvalGroup(evs)
    g.SetPrebinning(False)
    g.SetBucketing(False)     # (with it ordering, boxes and codes: the rows form)
    return evs, g, norms


def fill_ms(g, stream, evals, warmup):
    for _ in range(warmup):
        g.EvalAsync(False, stream)
    g.EvalFinished()
    g.Profile(True, 8 * evals)
    for _ in range(evals):
        g.EvalAsync(False, stream)
    g.EvalFinished()
    ms, launches = g.ProfileRead()
    g.Profile(False)
    return ms / evals, launches / evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--evals", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    w = workloads.config3(a.scale, nevents=1000)
    rng = np.random.default_rng(40)
    mult = [rng.integers(0, 81, size=s.samples.shape[0]).astype(np.uint32) for s in w.signals]
    params = DeviceArray(np.concatenate([np.ones(w.nsources), [0.01, 0.002, 0.01]]))
    stream = capi.new_stream()
    evw, gw, nw = build(w, mult, params, stream)
    evr, gr, nr = build(w, None, params, stream)
    rows = sum(s.samples.shape[0] for s in w.signals)
    out = dict(tool="weighted_fill_bench", rows=rows, mean_multiplicity=float(np.mean([m.mean() for m in mult])),
               multiplicity_total=int(sum(int(m.sum()) for m in mult)), evals=a.evals, warmup=a.warmup, repeats=[])
    for _ in range(a.repeats):
        tw, lw = fill_ms(gw, stream, a.evals, a.warmup)
        tr, lr = fill_ms(gr, stream, a.evals, a.warmup)
        out["repeats"].append(dict(weighted_us=1e3 * tw, rows_us=1e3 * tr, ratio=tw / tr, weighted_launches=lw,
                                   rows_launches=lr))
    bw, br = gw.AlgorithmicBytes()["fill_read"], gr.AlgorithmicBytes()["fill_read"]
    tws = [r["weighted_us"] for r in out["repeats"]]
    trs = [r["rows_us"] for r in out["repeats"]]
    out.update(weighted_bytes=bw, rows_bytes=br,
               weighted_us=float(np.mean(tws)), rows_us=float(np.mean(trs)), ratio=float(np.mean(tws) / np.mean(trs)),
               spread_weighted=float((max(tws) - min(tws)) / np.mean(tws)), spread_rows=float((max(trs) - min(trs)) / np.mean(trs)),
               weighted_share_of_peak=bw / (np.mean(tws) * 1e-6) / HBM_PEAK,
               rows_share_of_peak=br / (np.mean(trs) * 1e-6) / HBM_PEAK,
               weighted_norms_ok=bool(np.all(nw.get() > 0)), launch_info=gw.LaunchInfo().strip().splitlines())
    print(json.dumps(out))
    for e in evw + evr:
        e.close()
    gw.close()
    gr.close()


if __name__ == "__main__":
    main()
