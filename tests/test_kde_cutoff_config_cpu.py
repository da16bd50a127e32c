"""CPU: the configuration key "bandwidth_cutoff" of a kernel-density signal, read alike by sxmc_amd/io.py and
sxmc::load_config (config.h, through a dump driver built here) with the same message for every refusal; carried by the
workload's signals; and a configuration without the key loads exactly as before."""
import json
import math
import subprocess

import numpy as np
import pytest

from sxmc_amd import io, workloads
from tests.test_kde_sample_cpu import build_cpp, config_text


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("signal_cutoff_dump"), "signal_cutoff_dump")


def both(tmp_path, text, exe):
    """(python result, C++ result): each a list of (name, pdf, bandwidth_cutoff), or ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = [(s["name"], s["pdf"], float(s["bandwidth_cutoff"])) for s in fc.signals]
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        cpp = [(s["name"], s["pdf"], float(s["bandwidth_cutoff"])) for s in json.loads(r.stdout)["signals"]]
    else:
        assert r.returncode == 1 and r.stderr.startswith("signal_cutoff_dump: "), r.stderr
        cpp = ("error", r.stderr[len("signal_cutoff_dump: "):].strip())
    return py, cpp


def test_key_accepted_and_defaulted(tmp_path, dump):
    py, cpp = both(tmp_path, config_text(), dump)
    assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", 0.0)]                 # absent: no cutoff
    for v in (0, 1, 4, 6.5, 1.0000000000000002, 1e30):
        py, cpp = both(tmp_path, config_text(kernel={"bandwidth_cutoff": v}), dump)
        assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", float(v))]
    # a number that overflows to infinity in both parsers: R = +infinity
    text = config_text(kernel={"bandwidth_cutoff": "1e999"}).replace('"1e999"', "1e999")
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", math.inf)]
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_cutoff": 4, "bandwidth_sensitivity": 0.5,
                                                 "bandwidth_scale": [0.5, 2.0]}), dump)
    assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", 4.0)]


@pytest.mark.parametrize("hist,kernel,message", [
    ({"bandwidth_cutoff": 4}, None, 'signal \'flat\': "bandwidth_cutoff" is only for "pdf": "kernel"'),
    ({"pdf": "hist", "bandwidth_cutoff": 0}, None, 'signal \'flat\': "bandwidth_cutoff" is only for "pdf": "kernel"'),
    (None, {"pdf": None, "bandwidth_cutoff": 4}, 'signal \'line\': "bandwidth_cutoff" is only for "pdf": "kernel"'),
    (None, {"bandwidth_cutoff": 0.5}, 'signal \'line\': "bandwidth_cutoff" must be 0 or a number >= 1'),
    (None, {"bandwidth_cutoff": -3}, 'signal \'line\': "bandwidth_cutoff" must be 0 or a number >= 1'),
    (None, {"bandwidth_cutoff": 0.9999999999999999}, 'signal \'line\': "bandwidth_cutoff" must be 0 or a number >= 1'),
    (None, {"bandwidth_cutoff": "-1e999"}, None),
    (None, {"bandwidth_cutoff": "4"}, "bandwidth_cutoff: not a number"),
    (None, {"bandwidth_cutoff": [4]}, "bandwidth_cutoff: not a number"),
])
def test_key_refused_with_the_same_message(tmp_path, dump, hist, kernel, message):
    text = config_text(hist=hist, kernel=kernel)
    if message is None:      # minus infinity in both parsers
        text = text.replace('"-1e999"', "-1e999")
        message = 'signal \'line\': "bandwidth_cutoff" must be 0 or a number >= 1'
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == ("error", message)


def test_the_workload_carries_the_key(tmp_path):
    assert io.signal_cutoff("line", {}, "kernel") == 0.0 and io.signal_cutoff("flat", {}, "hist") == 0.0
    assert io.signal_cutoff("line", {"bandwidth_cutoff": 4}, "kernel") == 4.0
    s = workloads.Signal(np.zeros((3, 2), np.float32), 2, 1.0, 0)
    assert s.bandwidth_cutoff == 0.0
    rng = np.random.default_rng(3)
    for name, n in (("flat", 500), ("line", 200)):
        io.write_table(tmp_path / (name + ".npz"), np.stack([rng.uniform(0, 10, n), rng.uniform(0, 6, n)], axis=1),
                       ["e", "r"])
    (tmp_path / "fit.json").write_text(config_text(kernel={"bandwidth_cutoff": 4}))
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    assert [s.bandwidth_cutoff for s in w.signals] == [0.0, 4.0]
    (tmp_path / "fit.json").write_text(config_text())
    fc = io.load_config(str(tmp_path / "fit.json"))
    w = io.build_workload(fc)
    assert [s.bandwidth_cutoff for s in w.signals] == [0.0, 0.0]
    assert [s["bandwidth_cutoff"] for s in fc.signals] == [0.0, 0.0]
