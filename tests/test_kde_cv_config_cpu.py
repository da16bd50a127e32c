"""CPU: the configuration keys of cross-validated bandwidths -- "bandwidth_scale": "cv" and the optional object
"bandwidth_cv" on a "pdf": "kernel" signal -- read alike by sxmc_amd/io.py and sxmc::load_config (config.h, through a
dump driver built here) and refused alike, with the same messages; a configuration without the keys loads as before; the
workload carries the request to whoever builds the evaluators."""
import json
import subprocess

import numpy as np
import pytest

from sxmc_amd import io, pdfz, workloads
from tests.test_kde_sample_cpu import build_cpp, config_text

DEFAULTS = dict(lo=0.125, hi=4.0, steps=21, per_observable=True, max_rows=65536)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("signal_cv_dump"), "signal_cv_dump")


def both(tmp_path, text, exe):
    """(python result, C++ result): each a list of (name, pdf, bandwidth_scale, cv options or None), or
    ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = [(s["name"], s["pdf"], [float(v) for v in s["bandwidth_scale"]], s["bandwidth_cv"]) for s in fc.signals]
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        cpp = [(s["name"], s["pdf"], s["bandwidth_scale"],
                {k: s[k] for k in DEFAULTS} if s["cv"] else None) for s in json.loads(r.stdout)["signals"]]
    else:
        assert r.returncode == 1 and r.stderr.startswith("signal_cv_dump: "), r.stderr
        cpp = ("error", r.stderr[len("signal_cv_dump: "):].strip())
    return py, cpp


def test_keys_accepted_and_defaulted(tmp_path, dump):
    py, cpp = both(tmp_path, config_text(), dump)                                   # without the keys: as before
    assert py == cpp == [("flat", "hist", [], None), ("line", "kernel", [1.0, 1.0], None)]
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_scale": [0.5, 2.0]}), dump)
    assert py == cpp == [("flat", "hist", [], None), ("line", "kernel", [0.5, 2.0], None)]
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_scale": "cv"}), dump)
    assert py == cpp == [("flat", "hist", [], None), ("line", "kernel", [1.0, 1.0], DEFAULTS)]
    for given in ({}, {"lo": 0.25}, {"hi": 2, "steps": 7}, {"per_observable": False, "max_rows": 0},
                  {"lo": 0.5, "hi": 0.5, "steps": 1, "per_observable": 1, "max_rows": 1000},
                  {"steps": 32.0, "max_rows": 123456789}):
        py, cpp = both(tmp_path, config_text(kernel={"bandwidth_scale": "cv", "bandwidth_cv": given,
                                                     "bandwidth_sensitivity": 0.5}), dump)
        want = dict(DEFAULTS)
        want.update({k: (bool(v) if k == "per_observable" else v) for k, v in given.items()})
        assert py == cpp == [("flat", "hist", [], None), ("line", "kernel", [1.0, 1.0], want)], given
        assert py[1][3]["steps"] == want["steps"] and isinstance(py[1][3]["steps"], int)


LINE = "signal 'line': "


@pytest.mark.parametrize("hist,kernel,message", [
    ({"bandwidth_scale": "cv"}, None, 'signal \'flat\': "bandwidth_scale" is only for "pdf": "kernel"'),
    ({"bandwidth_cv": {}}, None, 'signal \'flat\': "bandwidth_cv" is only for "pdf": "kernel"'),
    (None, {"pdf": None, "bandwidth_cv": {"steps": 5}}, LINE + '"bandwidth_cv" is only for "pdf": "kernel"'),
    (None, {"bandwidth_scale": "scott"}, "bandwidth_scale: not a number"),
    (None, {"bandwidth_scale": "CV"}, "bandwidth_scale: not a number"),
    (None, {"bandwidth_scale": ["cv", "cv"]}, "bandwidth_scale: not a number"),
    (None, {"bandwidth_cv": {}}, LINE + '"bandwidth_cv" needs "bandwidth_scale": "cv"'),
    (None, {"bandwidth_scale": [1.0, 1.0], "bandwidth_cv": {"steps": 5}}, LINE + '"bandwidth_cv" needs "bandwidth_scale": "cv"'),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": [1, 2]}, LINE + '"bandwidth_cv" must be an object'),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"step": 5, "zz": 1}}, LINE + '"bandwidth_cv" has no key "step"'),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"steps": 0}}, LINE + "Cross-validation steps must be between 1 and 32."),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"steps": 33}}, LINE + "Cross-validation steps must be between 1 and 32."),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"steps": 2.5}}, "steps: not an integer"),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"steps": "21"}}, "steps: not a number"),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"lo": 0}}, LINE + "Cross-validation grid needs 0 < lo <= hi, both finite."),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"lo": 2, "hi": 1}}, LINE + "Cross-validation grid needs 0 < lo <= hi, both finite."),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"hi": "1e999"}}, None),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"lo": [0.1]}}, "lo: not a number"),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"per_observable": "yes"}}, "per_observable: not a boolean"),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"max_rows": -1}}, LINE + '"bandwidth_cv": "max_rows" must not be negative'),
    (None, {"bandwidth_scale": "cv", "bandwidth_cv": {"max_rows": 0.5}}, "max_rows: not an integer"),
])
def test_keys_refused_with_the_same_message(tmp_path, dump, hist, kernel, message):
    text = config_text(hist=hist, kernel=kernel)
    if message is None:      # a number that overflows to infinity in both parsers
        text = text.replace('"1e999"', "1e999")
        message = LINE + "Cross-validation grid needs 0 < lo <= hi, both finite."
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == ("error", message)


def test_the_workload_carries_the_request(tmp_path):
    s = workloads.Signal(np.zeros((3, 2), np.float32), 2, 1.0, 0)
    assert s.bandwidth_cv is None and s.cv_report is None
    assert io.signal_cv("line", {"pdf": "kernel", "bandwidth_scale": "cv"}, "kernel") == DEFAULTS
    assert io.signal_cv("line", {"pdf": "kernel", "bandwidth_scale": 2.0}, "kernel") is None
    assert io.signal_pdf("line", {"pdf": "kernel", "bandwidth_scale": "cv"}, 2) == ("kernel", [1.0, 1.0])
    assert pdfz.CvOptions(**DEFAULTS) == pdfz.CvOptions()
    rng = np.random.default_rng(3)
    for name, n in (("flat", 500), ("line", 200)):
        io.write_table(tmp_path / (name + ".npz"), np.stack([rng.uniform(0, 10, n), rng.uniform(0, 6, n)], axis=1),
                       ["e", "r"])
    (tmp_path / "fit.json").write_text(config_text(kernel={"bandwidth_scale": "cv", "bandwidth_cv": {"steps": 9}}))
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    want = dict(DEFAULTS, steps=9)
    assert [s.bandwidth_cv for s in w.signals] == [None, want] and w.signals[1].bandwidth_scale == [1.0, 1.0]
    (tmp_path / "fit.json").write_text(config_text())
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    assert [s.bandwidth_cv for s in w.signals] == [None, None]
