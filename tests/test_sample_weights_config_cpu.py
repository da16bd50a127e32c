"""CPU: a signal's "weight_field" (weighted Monte Carlo) read alike by sxmc_amd/io.py and sxmc::load_config (config.h,
through a dump driver built here): the same sample fields, multiplicities, n_mc and nexpected, the same message for every
refusal; a configuration without the key loads exactly as before."""
import json
import subprocess

import numpy as np
import pytest

from sxmc_amd import io
from tests import sample_weights_reference as ref
from tests.test_kde_sample_cpu import build_cpp


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("sample_weights_config_dump"), "sample_weights_config_dump")


def tables(tmp_path, weights=None):
    rng = np.random.default_rng(5)
    n = 200
    e_true = rng.uniform(0.0, 10.0, n)
    cols = {"e": e_true + rng.normal(0, 0.3, n), "r": rng.uniform(0.0, 7.0, n), "e_true": e_true,
            "w": rng.lognormal(0.0, 1.0, n) if weights is None else np.asarray(weights, np.float64)}
    fields = list(cols)
    io.write_table(str(tmp_path / "flat.npz"), np.stack([cols[f] for f in fields], axis=1).astype(np.float32), fields)
    io.write_table(str(tmp_path / "line.npz"), np.stack([cols[f] for f in fields], axis=1).astype(np.float32)[:50], fields)
    return {f: np.asarray(cols[f], np.float32) for f in fields}


def config_text(flat=None, line=None):
    f = {"title": "F", "filename": "flat.npz", "dataset": 0, "rate": 100.0, "systematics": ["e_res"]}
    g = {"title": "L", "filename": "line.npz", "dataset": 0, "rate": 40.0, "systematics": ["e_res"]}
    f.update(flat or {})
    g.update(line or {})
    for d in (f, g):
        for k in [k for k, v in d.items() if v is None]:
            del d[k]
    return json.dumps({
        "fit": {"nexperiments": 1, "nsteps": 10, "signals": ["flat", "line"], "observables": ["energy"], "cuts": ["radius"]},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 10, "min": 0.0, "max": 10.0},
                                 "radius": {"field": "r", "bins": 6, "min": 0.0, "max": 5.0}},
                 "systematics": {"e_res": {"type": "resolution_scale", "observable_field": "e", "truth_field": "e_true",
                                           "mean": [0.0], "sigma": [0.01]}}},
        "signals": {"flat": f, "line": g}})


def both(tmp_path, text, exe):
    """(python, C++): each {"sample_fields", "signals": [{name, n_mc, nexpected, log2_scale, rows, multiplicities}]} or
    ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        w = io.build_workload(fc)
        py = {"sample_fields": list(fc.sample_fields), "signals": [
            dict(name=s.name, n_mc=int(s.n_mc), nexpected=float(s.nexpected), log2_scale=int(s.weight_log2_scale),
                 rows=int(s.samples.shape[0]),
                 multiplicities=[] if s.multiplicities is None else [int(v) for v in s.multiplicities])
            for s in w.signals]}
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        cpp = json.loads(r.stdout)
    else:
        assert r.returncode == 1 and r.stderr.startswith("sample_weights_config_dump: "), r.stderr
        cpp = ("error", r.stderr[len("sample_weights_config_dump: "):].strip())
    return py, cpp


def test_weight_field_is_read_alike(tmp_path, dump):
    cols = tables(tmp_path)
    py, cpp = both(tmp_path, config_text(flat={"weight_field": "w"}), dump)
    assert py == cpp and not isinstance(py, tuple), (py, cpp)
    assert py["sample_fields"] == ["e", "e_true", "DATASET"]                     # the weight is not a sample field
    flat, line = py["signals"]
    m, k, total = ref.sample_multiplicities(cols["w"].astype(np.float64))        # over ALL rows of the file
    keep = ~((cols["r"] < 0.0) | (cols["r"] > 5.0))
    assert 0 < keep.sum() < keep.size
    assert flat["n_mc"] == total and flat["log2_scale"] == k and flat["rows"] == int(keep.sum())
    assert flat["multiplicities"] == [int(v) for v in m[keep]]                   # cut with the rows
    assert flat["nexpected"] == 100.0
    assert line == dict(name="line", n_mc=50, nexpected=40.0, log2_scale=0, rows=line["rows"], multiplicities=[])


def test_scale_uses_the_real_weight_total(tmp_path, dump):
    cols = tables(tmp_path)
    py, cpp = both(tmp_path, config_text(flat={"weight_field": "w", "rate": None, "scale": 4.0}), dump)
    assert py == cpp and not isinstance(py, tuple), (py, cpp)
    m, k, total = ref.sample_multiplicities(cols["w"].astype(np.float64))
    want = float(np.float32(-1.0) / np.float32(4.0)) * (-1.0 * float(np.ldexp(float(total), -k)))
    assert py["signals"][0]["nexpected"] == want and abs(want - cols["w"].astype(np.float64).sum() / 4.0) < 1e-3 * want


def test_config_without_the_key_loads_as_before(tmp_path, dump):
    tables(tmp_path)
    py, cpp = both(tmp_path, config_text(), dump)
    assert py == cpp and not isinstance(py, tuple)
    assert [s["multiplicities"] for s in py["signals"]] == [[], []] and [s["n_mc"] for s in py["signals"]] == [200, 50]
    assert [s["log2_scale"] for s in py["signals"]] == [0, 0]


@pytest.mark.parametrize("flat,weights,message", [
    ({"weight_field": "nope"}, None, "signal 'flat': weight_field 'nope' is not a field of flat.npz"),
    ({"weight_field": "e"}, None, "signal 'flat': weight_field 'e' is also an observable or a systematic's field"),
    ({"weight_field": "e_true"}, None, "signal 'flat': weight_field 'e_true' is also an observable or a systematic's field"),
    ({"weight_field": "w", "pdf": "kernel"}, None,
     'signal \'flat\': "weight_field" is only for "pdf": "hist" (kernel-density weights are not built)'),
    ({"weight_field": "w"}, "negative", "signal 'flat': weight_field 'w': sample weights: the weight of row 7 is negative or not finite"),
    ({"weight_field": "w"}, "nan", "signal 'flat': weight_field 'w': sample weights: the weight of row 7 is negative or not finite"),
    ({"weight_field": 3}, None, "weight_field: not a string"),
])
def test_refusals_have_the_same_message(tmp_path, dump, flat, weights, message):
    w = None
    if weights is not None:
        w = np.ones(200)
        w[7] = -1.0 if weights == "negative" else np.nan
    tables(tmp_path, w)
    py, cpp = both(tmp_path, config_text(flat=flat), dump)
    assert py == cpp == ("error", message)
