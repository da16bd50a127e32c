"""GPU: a fit configuration whose kernel-density signal carries "bandwidth_cutoff": 4, end to end.  The Python layers
(load_config, build_workload, make_evaluators, make_fake_dataset, fit_spectra) apply the cutoff and leave the fake data
and the fit spectra those of the same configuration without the key (the sampler and the projection do not see it);
the C++ layers (load_config, build_pdfz, share_pdfz, sxmc::MCMC) walk the mixed fit in the reference's call sequence
and in the mixed form to the same chain bytes, culling tiles on the way."""
import json
import subprocess

import numpy as np
import pytest

from sxmc_amd import ensemble, io, pdfz
from tests.test_kde_sample_cpu import build_cpp

pytestmark = pytest.mark.gpu


def write_config(tmp_path, cutoff, name):
    rng = np.random.default_rng(27)
    n1, n2 = 20000, 3000
    t1 = 10 * rng.random(n1) * rng.random(n1)
    t2 = np.concatenate([rng.normal(3.0, 0.15, n2 // 2), rng.normal(7.0, 0.3, n2 - n2 // 2)])
    io.write_table(tmp_path / "spectrum.npz", np.stack([t1 + rng.normal(0, 0.2, n1), t1], axis=1), ["e", "e_true"])
    io.write_table(tmp_path / "lines.npz", np.stack([t2 + rng.normal(0, 0.1, n2), t2], axis=1), ["e", "e_true"])
    lines = {"filename": "lines.npz", "dataset": 0, "rate": 300.0, "systematics": ["e_scale"], "pdf": "kernel",
             "bandwidth_scale": 0.5}
    if cutoff is not None:
        lines["bandwidth_cutoff"] = cutoff
    cfg = {
        "fit": {"nexperiments": 1, "nsteps": 300, "seed": 31, "burnin_fraction": 0.2,
                "signals": ["spectrum", "lines"], "observables": ["energy"], "signal_name": "lines"},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 25, "min": 0.0, "max": 10.0}},
                 "systematics": {"e_scale": {"type": "scale", "observable_field": "e", "mean": [0.0],
                                             "sigma": [0.02]}}},
        "signals": {"spectrum": {"filename": "spectrum.npz", "dataset": 0, "rate": 600.0, "systematics": ["e_scale"]},
                    "lines": lines}}
    path = tmp_path / (name + ".json")
    path.write_text(json.dumps(cfg))
    return path


def test_a_configuration_with_a_cutoff_end_to_end(tmp_path):
    w = io.build_workload(io.load_config(str(write_config(tmp_path, 4, "fit_cut"))))
    w0 = io.build_workload(io.load_config(str(write_config(tmp_path, None, "fit_plain"))))
    assert [s.bandwidth_cutoff for s in w.signals] == [0.0, 4.0]
    assert [s.bandwidth_cutoff for s in w0.signals] == [0.0, 0.0]
    evs, evs0 = ensemble.make_evaluators(w), ensemble.make_evaluators(w0)
    assert isinstance(evs[1], pdfz.EvalKernel) and evs[1].Cutoff() == 4.0 and evs0[1].Cutoff() == 0.0
    assert evs[1].Bandwidths().tobytes() == evs0[1].Bandwidths().tobytes()
    rows, observed = ensemble.make_fake_dataset(np.random.default_rng(9), w, evs)
    rows0, observed0 = ensemble.make_fake_dataset(np.random.default_rng(9), w0, evs0)
    assert list(observed) == list(observed0) and observed[1] > 100 and rows.tobytes() == rows0.tobytes()
    means = np.concatenate([np.ones(w.nsources), np.zeros(w.nparameters - w.nsources)])
    a, b = ensemble.fit_spectra(w, evs, means, rows), ensemble.fit_spectra(w0, evs0, means, rows0)
    assert np.asarray(a[0]["signals"][1]["spectrum"]).tobytes() == np.asarray(b[0]["signals"][1]["spectrum"]).tobytes()

    exe = build_cpp(tmp_path, "kde_cutoff_fit")
    r = subprocess.run([exe, str(tmp_path / "fit_cut.json")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kernels"] == [{"name": "lines", "signal_cutoff": 4, "cutoff": 4, "shared_cutoff": 4}]
    ref, mixed = out["walks"]
    assert ref["form"] == "reference" and mixed["form"] == "mixed" and out["same_bytes"]
    assert ref["rows"] == mixed["rows"] > 0 and ref["finite_nll_rows"] == ref["rows"] and ref["accepted"] > 0
    for walk in (ref, mixed):
        (visited, possible), = walk["tiles"]
        assert 0 < visited < possible                   # two lines 4 units apart: tiles are culled in the walk itself
    for e in evs + evs0:
        e.close()
