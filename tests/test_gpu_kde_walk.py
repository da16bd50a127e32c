"""GPU: the mixed histogram + kernel-density walk of tests/cpp/test_kde_walk.cpp (sxmc::MCMC's per-evaluator path)
checked against the host.  About 20 recorded rows spread along the chain are recomputed: the histogram signal with the
oracle, the kernel signal with the f64 reference, the NLL with oracle.full_nll.  The tolerance is the float rounding of
the recorded row (its NLL, and its parameters through the NLL's change when each moves by half a float ulp) plus the
kernel values' error bound propagated through the log-sum."""
import json
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.kde_reference import U, ref_kde
from tests.test_gpu_pdfz import oracle_eval
from tests.test_kde_cpu import build_kde_walk

pytestmark = pytest.mark.gpu


def full_nll(ix, lut, norms, pars):
    return oracle.full_nll(lut, pars, lut.shape[1], 2, ix["nsources"], np.array(ix["means"]), np.array(ix["sigmas"]),
                           np.array(ix["nexpected"]), np.array(ix["n_mc"], np.uint32),
                           np.array(ix["source_id"], np.int16), norms)[0]


def host_nll(ix, arrays, pars):
    """(NLL, its error from the kernel values' bound, lookup table, norms) at the parameters `pars` (f64)."""
    ns = ix["nsources"]
    systs = ix["systematics"]
    sp = pars[ns:]
    data = arrays["data"]
    h = oracle_eval(arrays["flat"].ravel(), ix["nfields"], ix["lower"], ix["upper"], ix["bins"], systs, sp,
                    points=data.ravel())
    k = ref_kde(arrays["line"].ravel(), ix["nfields"], 1, ix["lower"], ix["upper"], ix["bandwidth_scale"], systs,
                dict(enumerate(sp)), data.ravel())
    assert np.allclose(k.h, ix["bandwidth"], rtol=1e-12)
    ne = len(data)
    lut = np.stack([h["out"][:ne], k.values.astype(np.float32)])
    norms = np.array([h["norm"], k.norm], np.uint32)
    # d log s_i = c_kde dv_i / s_i, with s_i the event's sum as nll_kernels forms it (f32 efficiency)
    nexp, n_mc, sid = np.array(ix["nexpected"]), np.array(ix["n_mc"], np.uint32), np.array(ix["source_id"])
    eff = (1.0 * norms / n_mc).astype(np.float32).astype(np.float64)
    c = pars[sid] * nexp * eff
    s = c @ np.nan_to_num(lut.astype(np.float64))
    dv = k.bound + U * np.abs(np.nan_to_num(k.values))        # (+ the reference's own rounding to float)
    dv = np.where(np.isnan(k.values), 0.0, dv)
    err = float(np.sum(np.where(s > 0, c[1] * dv / np.where(s > 0, s, 1.0), 0.0)))
    return full_nll(ix, lut, norms, pars), err, lut, norms


def run_walk(tmp_path):
    exe = build_kde_walk(tmp_path)
    r = subprocess.run([exe, "3000", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"]
    ix = json.loads((tmp_path / "index.json").read_text())
    arrays = {k: np.fromfile(tmp_path / f, dtype="<f4").reshape(n, m) for k, (f, n, m) in ix["arrays"].items()}
    assert arrays["chain"].shape[0] == line["rows"]
    return ix, arrays


def check_rows(ix, arrays, nrows=20):
    chain = arrays["chain"]
    assert chain.shape[0] > nrows and chain.shape[1] == len(ix["names"]) == len(ix["means"]) + 1
    rows = np.unique(np.linspace(0, len(chain) - 1, nrows).round().astype(int))
    worst = 0.0
    ns = ix["nsources"]
    for r in rows:
        pars = chain[r, :-1].astype(np.float64)
        rec = float(chain[r, -1])
        nll, kerr, lut, norms = host_nll(ix, arrays, pars)
        # the recorded parameters are floats: the NLL's change over half a float ulp of each, either way (a source
        # rate leaves the lookup table as it is)
        perr = 0.0
        for q in range(len(pars)):
            half = float(np.spacing(np.float32(abs(pars[q])))) / 2
            moved = []
            for d in (-half, half):
                p = pars.copy()
                p[q] += d
                moved.append(host_nll(ix, arrays, p)[0] if q >= ns else full_nll(ix, lut, norms, p))
            perr += max(abs(m - nll) for m in moved)
        tol = float(np.spacing(np.float32(abs(rec)))) / 2 + perr + kerr + 1e-12 * abs(nll) * len(arrays["data"])
        worst = max(worst, abs(nll - rec) / tol)
        print("row %d: recorded %.9g host %.9g |diff| %.3g tolerance %.3g (parameters %.3g, kernel values %.3g)"
              % (r, rec, nll, abs(nll - rec), tol, perr, kerr))
        assert abs(nll - rec) <= tol, (r, rec, nll, tol)
    print("walk: worst |recorded - host| / tolerance %.3g over %d rows" % (worst, len(rows)))
    return worst


def test_recorded_nlls_agree_with_the_host(tmp_path):
    ix, arrays = run_walk(tmp_path)
    check_rows(ix, arrays)
    # power: the same rows against a walk whose kernel signal had the wrong bandwidth fail
    wrong = dict(ix, bandwidth_scale=[1.01])
    wrong["bandwidth"] = [ix["bandwidth"][0] * 1.01]
    with pytest.raises(AssertionError):
        check_rows(wrong, arrays, nrows=3)
