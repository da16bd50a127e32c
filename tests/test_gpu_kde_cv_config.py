"""GPU: a fit configuration with "bandwidth_scale": "cv" end to end.  The Python layers (load_config, build_workload,
make_evaluators) and the C++ ones (load_config, build_pdfz) choose the scales the reference chooses
(tests/kde_cv_reference.py; the case is one of its gap-checked selection cases) and build the same evaluator; from then
on the signal carries the numbers: a second evaluator, the fake data, the fit spectra and a short mixed walk are those
of the same configuration with the numbers typed in."""
import json
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import ensemble, io, pdfz
from tests import kde_cv_reference as cv
from tests.test_kde_sample_cpu import build_cpp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_config(tmp_path, scale, name):
    rng = np.random.default_rng(5)
    n1 = 20000
    t1 = 10 * rng.random(n1) * rng.random(n1)
    io.write_table(tmp_path / "spectrum.npz", np.stack([t1 + rng.normal(0, 0.2, n1), t1], axis=1), ["e", "e_true"])
    io.write_table(tmp_path / "line.npz", cv.config_line_table(), ["e", "e_true"])
    line = {"filename": "line.npz", "dataset": 0, "rate": 300.0, "systematics": ["e_scale"], "pdf": "kernel",
            "bandwidth_scale": scale, "bandwidth_sensitivity": 0.25}
    if scale == "cv":
        line["bandwidth_cv"] = dict(cv.CONFIG_CV)
    cfg = {
        "fit": {"nexperiments": 1, "nsteps": 400, "seed": 31, "burnin_fraction": 0.2,
                "signals": ["spectrum", "line"], "observables": ["energy"], "signal_name": "line"},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 25, "min": 0.0, "max": 10.0}},
                 "systematics": {"e_scale": {"type": "scale", "observable_field": "e", "mean": [0.0],
                                             "sigma": [0.02]}}},
        "signals": {"spectrum": {"filename": "spectrum.npz", "dataset": 0, "rate": 600.0, "systematics": ["e_scale"]},
                    "line": line}}
    path = tmp_path / (name + ".json")
    path.write_text(json.dumps(cfg))
    return path


def run_fit(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_a_configuration_with_cross_validated_scales_end_to_end(tmp_path):
    x, D, lower, upper, o = cv.selection_cases()["config_line"]
    want = cv.select(x.ravel(), 1, D, lower, upper, o)
    assert want["rows_used"] <= cv.CONFIG_CV["max_rows"] < len(x) and want["scale"][0] < 1.0

    # Python: the first evaluator built for the signal searches; the signal then carries the numbers
    w = io.build_workload(io.load_config(str(write_config(tmp_path, "cv", "fit_cv"))))
    assert w.signals[1].bandwidth_cv == dict(cv.CONFIG_CV, per_observable=True) and w.signals[0].bandwidth_cv is None
    evs = ensemble.make_evaluators(w)
    line = evs[1]
    assert isinstance(line, pdfz.EvalKernel) and np.array_equal(line.BandwidthScale(), want["scale"])
    rep = line.CvReport()
    assert rep.rows_used == want["rows_used"] and rep.at_edge == list(want["at_edge"])
    assert w.signals[1].bandwidth_scale == list(want["scale"]) and w.signals[1].bandwidth_cv is None
    assert w.signals[1].cv_report is rep and line.BandwidthSensitivity() == 0.25
    again = ensemble.make_evaluators(w)                         # typed in now: no second search
    assert again[1].CvReport() is None and again[1].Bandwidths().tobytes() == line.Bandwidths().tobytes()
    assert again[1].LocalFactors().tobytes() == line.LocalFactors().tobytes()

    # the same configuration with the numbers typed in: the same evaluator, fake data and fit spectra
    wt = io.build_workload(io.load_config(str(write_config(tmp_path, [float(want["scale"][0])], "fit_typed"))))
    evt = ensemble.make_evaluators(wt)
    assert evt[1].Bandwidths().tobytes() == line.Bandwidths().tobytes()
    assert evt[1].LocalFactors().tobytes() == line.LocalFactors().tobytes()
    rows, observed = ensemble.make_fake_dataset(np.random.default_rng(9), w, evs)
    rows_t, observed_t = ensemble.make_fake_dataset(np.random.default_rng(9), wt, evt)
    assert list(observed) == list(observed_t) and observed[1] > 100 and rows.tobytes() == rows_t.tobytes()
    means = np.concatenate([np.ones(w.nsources), np.zeros(w.nparameters - w.nsources)])
    a, b = ensemble.fit_spectra(w, evs, means, rows), ensemble.fit_spectra(wt, evt, means, rows_t)
    assert np.asarray(a[0]["signals"][1]["spectrum"]).tobytes() == np.asarray(b[0]["signals"][1]["spectrum"]).tobytes()
    shared = pdfz.EvalKernel.Shared(line)
    assert np.array_equal(shared.BandwidthScale(), want["scale"]) and shared.CvReport() is rep

    # C++: the same choice, the same bandwidths, and the walk of the configuration with the numbers typed in
    exe = build_cpp(tmp_path, "kde_cv_fit")
    got = run_fit(exe, tmp_path / "fit_cv.json")
    typed = run_fit(exe, tmp_path / "fit_typed.json")
    k, kt = got["kernels"][0], typed["kernels"][0]
    assert k["name"] == "line" and k["searched"] and not k["pending"] and k["rows_used"] == want["rows_used"]
    assert not kt["searched"] and not kt["pending"]
    assert k["scale"] == k["signal_scale"] == kt["scale"] == list(want["scale"])
    assert k["bandwidths"] == kt["bandwidths"] == list(line.Bandwidths())
    assert got["walk"] == typed["walk"] and got["walk"]["accepted"] > 0 and got["walk"]["nevents"] > 0
    for e in evs + again + evt + [shared]:
        e.close()
