"""GPU tests of pdfz::EvalKernel, the kernel-density PDF, against a numpy f64 restatement of its contract
(sxmc_amd/include/sxmc/pdfz.h, class EvalKernel; tests/kde_reference.py): values, norm, special points, normalisation, bandwidths,
determinism, fill-only evaluation, launch shapes, the NLL over a mixed lookup table, the C++ walk and the tool."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import nll, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests.kde_reference import check_values, ref_bandwidths, ref_kde
from tests.test_kde_cpu import build_kde_walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def gpu_kde(samples, nfields, nobs, lower, upper, scale, systs, params, points, dataset=0, par_off=0, par_stride=1,
            pdf_off=0, pdf_stride=1, norm_off=0, do_eval_pdf=True, repeat=1, ev=None):
    if ev is None:
        ev = pdfz.EvalKernel(samples, nfields, nobs, lower, upper, scale, dataset=dataset)
        for s in systs:
            ev.AddSystematic(make_systematic(s))
    points = np.ascontiguousarray(points, np.float32)
    ev.SetEvalPoints(points)
    npts = points.size // (nobs + 1)
    pbuf = np.full(par_off + par_stride * (max(params.keys(), default=0) + 1) + 1, 7.5, np.float64)
    for q, v in params.items():
        pbuf[par_off + par_stride * q] = v
    pdf = DeviceArray(np.full(pdf_off + pdf_stride * max(npts, 1), 12345.0, np.float32))
    norm = DeviceArray(np.full(norm_off + 2, 99, np.uint32))
    par = DeviceArray(pbuf)
    ev.SetPDFValueBuffer(pdf, pdf_off, pdf_stride)
    ev.SetNormalizationBuffer(norm, norm_off)
    ev.SetParameterBuffer(par, par_off, par_stride)
    outs = []
    for _ in range(repeat):
        ev.EvalAsync(do_eval_pdf)
        ev.EvalFinished()
        outs.append((pdf.get(), norm.get()))
    raw, nv = outs[-1]
    vals = raw[pdf_off::pdf_stride][:npts] if pdf_stride > 0 else raw
    return dict(ev=ev, values=vals, raw=raw, norm=int(nv[norm_off]), norms=nv, outs=outs)


SYSTS_2D = [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=1, pars=[1, 2]),
            dict(type="resolution_scale", obs=0, true_obs=2, pars=[3]), dict(type="ctscale", obs=1, pars=[4])]
PARAMS_2D = {0: 0.05, 1: 0.02, 2: -0.003, 3: 0.1, 4: -0.04}


def table_2d(rng, n):
    t = rng.normal(2.0, 0.8, n)
    return np.stack([t + rng.normal(0, 0.3, n), rng.uniform(-1.2, 1.2, n), t], axis=1).astype(np.float32).ravel()


def points_2d(rng, n):
    p = np.stack([rng.uniform(-0.5, 4.5, n), rng.uniform(-1.1, 1.1, n), np.zeros(n)], axis=1)
    return p.astype(np.float32).ravel()


# ------------------------------------------------------------------ tests
def test_values_1d_shift_scale():
    rng = np.random.default_rng(1)
    n = 3000
    t = rng.exponential(1.5, n)
    samples = np.stack([t + rng.normal(0, 0.2, n), t], axis=1).astype(np.float32).ravel()
    systs = [dict(type="scale", obs=0, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=1, pars=[1])]
    params = {0: 0.03, 1: -0.2}
    pts = np.stack([rng.uniform(-0.2, 6.2, 500), np.zeros(500)], axis=1).astype(np.float32).ravel()
    ref = ref_kde(samples, 2, 1, [0.0], [6.0], [0.8], systs, params, pts)
    got = gpu_kde(samples, 2, 1, [0.0], [6.0], [0.8], systs, params, pts, par_off=2, par_stride=3, pdf_off=5,
                  pdf_stride=2, norm_off=1)
    assert got["norm"] == ref.norm
    check_values(got["values"], ref, "1-D")
    assert np.all(got["raw"][:5] == 12345.0) and np.all(got["raw"][6::2] == 12345.0)   # only the strided slots


def test_values_2d_all_systematics():
    rng = np.random.default_rng(2)
    samples = table_2d(rng, 4000)
    pts = points_2d(rng, 400)
    ref = ref_kde(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.0, 0.7], SYSTS_2D, PARAMS_2D, pts)
    got = gpu_kde(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.0, 0.7], SYSTS_2D, PARAMS_2D, pts, par_off=1,
                  par_stride=2, pdf_off=3, pdf_stride=3, norm_off=1)
    assert got["norm"] == ref.norm
    check_values(got["values"], ref, "2-D")


def test_norm_bit_equal_to_evalhist():
    rng = np.random.default_rng(3)
    samples = table_2d(rng, 20000)
    pts = points_2d(rng, 50)
    for params in (PARAMS_2D, {0: -0.3, 1: 0.1, 2: 0.01, 3: 0.4, 4: 0.2}):
        got = gpu_kde(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.0, 1.0], SYSTS_2D, params, pts, par_off=1,
                      par_stride=2)
        hist = pdfz.EvalHist(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [37, 11])
        for s in SYSTS_2D:
            hist.AddSystematic(make_systematic(s))
        pbuf = np.full(1 + 2 * 6, 7.5)
        for q, v in params.items():
            pbuf[1 + 2 * q] = v
        norm, par = DeviceArray(np.zeros(1, np.uint32)), DeviceArray(pbuf)
        hist.SetNormalizationBuffer(norm, 0)
        hist.SetParameterBuffer(par, 1, 2)
        hist.EvalAsync(False)
        hist.EvalFinished()
        assert got["norm"] == int(norm.get()[0])
        hist.close()


def test_special_points_and_empty_domain():
    rng = np.random.default_rng(4)
    samples = rng.uniform(0.1, 0.9, 500).astype(np.float32)
    pts = np.array([[0.5, 1], [0.5, 0], [1.5, 1], [1.5, 0], [np.nan, 1], [-0.1, 0], [0.0, 1]], np.float32).ravel()
    got = gpu_kde(samples, 1, 1, [0.0], [1.0], [1.0], [dict(type="shift", obs=0, pars=[0])], {0: 0.0}, pts,
                  dataset=1)
    v = got["values"]
    assert v[0] > 0 and v[1] == 0.0 and math.isnan(v[2]) and math.isnan(v[3]) and math.isnan(v[4])
    assert math.isnan(v[5]) and v[6] > 0
    # every sample shifted out of the domain: norm 0, in-domain points of the data set NaN, of another data set 0
    got = gpu_kde(samples, 1, 1, [0.0], [1.0], [1.0], [dict(type="shift", obs=0, pars=[0])], {0: 5.0}, pts,
                  dataset=1, ev=got["ev"])
    v = got["values"]
    assert got["norm"] == 0
    assert math.isnan(v[0]) and v[1] == 0.0 and math.isnan(v[2]) and math.isnan(v[3])


def test_normalisation_1d_and_2d():
    rng = np.random.default_rng(5)
    # samples crowd both edges: the truncation weights matter
    x = np.concatenate([rng.beta(0.6, 3.0, 1500), rng.beta(3.0, 0.6, 1500)]).astype(np.float32)
    g = 20000
    grid = ((np.arange(g) + 0.5) / g).astype(np.float32)
    pts = np.stack([grid, np.zeros(g)], axis=1).astype(np.float32).ravel()
    v = gpu_kde(x, 1, 1, [0.0], [1.0], [1.0], [], {}, pts)["values"]
    integral = float(np.sum(v.astype(np.float64)) / g)
    print("1-D integral %.8f" % integral)
    assert abs(integral - 1.0) <= 1e-4
    s2 = np.stack([rng.beta(0.7, 2.0, 2000), rng.beta(2.0, 0.7, 2000)], axis=1).astype(np.float32).ravel()
    m = 400
    c = (np.arange(m) + 0.5) / m
    gx, gy = np.meshgrid(c, 2 * c - 1, indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(m * m)], axis=1).astype(np.float32).ravel()
    v = gpu_kde(s2, 2, 2, [0.0, -1.0], [1.0, 1.0], [1.0, 1.0], [], {}, pts)["values"]
    integral = float(np.sum(v.astype(np.float64)) * (1.0 / m) * (2.0 / m))
    print("2-D integral %.8f" % integral)
    assert abs(integral - 1.0) <= 1e-3


def test_bandwidths_scott():
    rng = np.random.default_rng(6)
    samples = table_2d(rng, 5000)
    ev = pdfz.EvalKernel(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.3, 0.6])
    want = ref_bandwidths(samples, 3, 2, np.array([0.0, -1.0]), np.array([4.0, 1.0]), [1.3, 0.6])
    assert np.allclose(ev.Bandwidths(), want, rtol=1e-12, atol=0)
    assert ev.nsamples == 5000
    ev.close()


def test_determinism_and_fill_only():
    rng = np.random.default_rng(7)
    samples = table_2d(rng, 30000)
    pts = points_2d(rng, 3000)
    got = gpu_kde(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.0, 1.0], SYSTS_2D, PARAMS_2D, pts, repeat=3)
    first = got["outs"][0]
    for pdf, norm in got["outs"][1:]:
        assert pdf.tobytes() == first[0].tobytes() and np.array_equal(norm, first[1])
    fill = gpu_kde(samples, 3, 2, [0.0, -1.0], [4.0, 1.0], [1.0, 1.0], SYSTS_2D, PARAMS_2D, pts, do_eval_pdf=False,
                   ev=got["ev"])
    assert np.all(fill["raw"] == 12345.0)
    assert fill["norm"] == got["norm"] > 0


@pytest.mark.parametrize("npoints,nsamples", [(7, 1000000), (1000000, 33), (1000, 1000)])
def test_shapes(npoints, nsamples):
    rng = np.random.default_rng(npoints + nsamples)
    samples = rng.normal(0.5, 0.2, nsamples).astype(np.float32)
    pts = np.stack([rng.uniform(-0.1, 1.1, npoints), np.zeros(npoints)], axis=1).astype(np.float32).ravel()
    ref = ref_kde(samples, 1, 1, [0.0], [1.0], [1.0], [], {}, pts)
    got = gpu_kde(samples, 1, 1, [0.0], [1.0], [1.0], [], {}, pts)
    assert got["norm"] == ref.norm
    check_values(got["values"], ref, "E=%d N=%d" % (npoints, nsamples))


def test_nll_over_mixed_lut():
    rng = np.random.default_rng(8)
    ne = 2000
    big = rng.normal(2.0, 1.0, 100000).astype(np.float32)
    small = rng.normal(1.0, 0.3, 800).astype(np.float32)
    events = np.stack([np.concatenate([rng.normal(2.0, 1.0, ne // 2), rng.normal(1.0, 0.3, ne // 2)]),
                       np.zeros(ne)], axis=1).astype(np.float32)
    events[:, 0] = np.clip(events[:, 0], 0.0, 3.999)
    lut = DeviceArray(np.zeros(2 * ne, np.float32))
    norms = DeviceArray(np.zeros(2, np.uint32))
    pars = np.array([1.1, 0.9, 0.01])
    dpars = DeviceArray(pars)
    hist = pdfz.EvalHist(big, 1, 1, [0.0], [4.0], [40])
    kde = pdfz.EvalKernel(small, 1, 1, [0.0], [4.0], [1.0])
    for j, ev in enumerate((hist, kde)):
        ev.AddSystematic(pdfz.ScaleSystematic(0, [0]))
        ev.SetEvalPoints(events.ravel())
        ev.SetPDFValueBuffer(lut, j * ne, 1)
        ev.SetNormalizationBuffer(norms, j)
        ev.SetParameterBuffer(dpars, 2, 1)
    for ev in (hist, kde):
        ev.EvalAsync()
    for ev in (hist, kde):
        ev.EvalFinished()
    host_lut = lut.get().reshape(2, ne)
    ref = ref_kde(small, 1, 1, [0.0], [4.0], [1.0], [dict(type="scale", obs=0, pars=[0])], {0: 0.01},
                  events.ravel())
    check_values(host_lut[1], ref, "KDE row of the mixed LUT")
    assert int(norms.get()[1]) == ref.norm
    nexp = np.array([1000.0, 1000.0])
    n_mc = np.array([100000, 800], np.uint32)
    sid = np.array([0, 1], np.int16)
    means, sigmas = np.array([1.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.02])
    d = {k: DeviceArray(v) for k, v in dict(nexpected=nexp, n_mc=n_mc, source_id=sid, means=means,
                                                sigmas=sigmas).items()}
    grid, block = 4, 128
    sums = DeviceArray.zeros(grid * block, np.float64)
    total = DeviceArray.zeros(1, np.float64)
    out = DeviceArray.zeros(1, np.float64)
    nll.nll_event_chunks(grid, block, None, lut, dpars, ne, 2, d["nexpected"], d["n_mc"], d["source_id"], norms, sums)
    nll.nll_event_reduce(1, 128, None, grid * block, sums, total)
    nll.nll_total(1, 1, None, 3, dpars, 2, 2, d["means"], d["sigmas"], total, d["nexpected"], d["n_mc"],
                  d["source_id"], norms, out)
    got = out.get()[0]
    # numpy: the NLL of nll_kernels.cpp over the lookup table the evaluators wrote
    want, _ = oracle.full_nll(host_lut.astype(np.float32), pars, ne, 2, 2, means, sigmas, nexp, n_mc, sid,
                              norms.get())
    print("NLL gpu %.12g numpy %.12g" % (got, want))
    assert abs(got - want) <= 1e-6 * abs(want)
    hist.close()
    kde.close()


def test_cpp_walk_with_kde_signal(tmp_path):
    exe = build_kde_walk(tmp_path)
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and 0 < line["acceptance"] < 1 and line["rows"] == line["finite_nll_rows"] > 0


def test_kde_bench_tool_small():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kde_bench.py"), "--samples", "4096",
                        "--points", "2000", "--seconds", "0.2", "--cpu-points", "50"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("ms_per_eval", "pairs_per_s", "bound_pairs_per_s", "fraction_of_bound", "cpu_numpy_pairs_per_s"):
        assert k in line and line[k] > 0, k
