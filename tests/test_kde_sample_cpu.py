"""CPU: the configuration keys of kernel-density signals ("pdf", "bandwidth_scale") read alike by sxmc_amd/io.py and
sxmc::load_config (config.h, through a dump driver built here), with the same messages for every refusal; the new C ABI
entry points (sampling, shared evaluators) declared, exported, in the ctypes table and refusing null arguments without
a device; the Python MCMC refusing a kernel-density signal before any device work."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, io, workloads
from sxmc_amd.mcmc import MCMC
from tests.test_abi import declared_symbols, exported
from tests.test_kde_cpu import cpp_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"sxmc_kde_random_sample", "sxmc_kde_create_shared", "sxmc_kde_sample_pool"}


def build_cpp(outdir, name):
    """tests/cpp/<name>.cpp built with the C++ tests' flags into outdir."""
    cxx, ld = cpp_flags()
    exe = os.path.join(str(outdir), name)
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    subprocess.run(["g++"] + cxx + ["-o", exe, src] + ld, check=True, capture_output=True, text=True, timeout=600)
    return exe


def config_text(hist=None, kernel=None, observables=("energy", "radius")):
    """Two signals: "flat" (a histogram unless `hist` says more) and "line" (`kernel` keys, default pdf kernel)."""
    flat = {"title": "F", "filename": "flat.npz", "dataset": 0, "rate": 100.0, "systematics": ["e_scale"]}
    line = {"title": "L", "filename": "line.npz", "dataset": 0, "rate": 40.0, "systematics": ["e_scale"],
            "pdf": "kernel"}
    flat.update(hist or {})
    line.update(kernel or {})
    for d in (flat, line):
        for k in [k for k, v in d.items() if v is None]:
            del d[k]
    return json.dumps({
        "fit": {"nexperiments": 2, "nsteps": 100, "signals": ["flat", "line"], "observables": list(observables)},
        "pdfs": {"observables": {"energy": {"field": "e", "bins": 10, "min": 0.0, "max": 10.0},
                                 "radius": {"field": "r", "bins": 6, "min": 0.0, "max": 6.0}},
                 "systematics": {"e_scale": {"type": "scale", "observable_field": "e", "mean": [0.0],
                                             "sigma": [0.01]}}},
        "signals": {"flat": flat, "line": line}})


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("signal_pdf_dump"), "signal_pdf_dump")


def both(tmp_path, text, exe):
    """(python result, C++ result): each a list of (name, pdf, bandwidth_scale), or ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = [(s["name"], s["pdf"], [float(v) for v in s["bandwidth_scale"]]) for s in fc.signals]
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        cpp = [(s["name"], s["pdf"], s["bandwidth_scale"]) for s in json.loads(r.stdout)["signals"]]
    else:
        assert r.returncode == 1 and r.stderr.startswith("signal_pdf_dump: "), r.stderr
        cpp = ("error", r.stderr[len("signal_pdf_dump: "):].strip())
    return py, cpp


def test_config_keys_agree_between_python_and_cpp(tmp_path, dump):
    py, cpp = both(tmp_path, config_text(), dump)
    assert py == cpp == [("flat", "hist", []), ("line", "kernel", [1.0, 1.0])]          # defaults
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_scale": [0.5, 2.25]}), dump)
    assert py == cpp == [("flat", "hist", []), ("line", "kernel", [0.5, 2.25])]         # fit-observable order
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_scale": 0.75}), dump)
    assert py == cpp == [("flat", "hist", []), ("line", "kernel", [0.75, 0.75])]        # one number for all
    py, cpp = both(tmp_path, config_text(hist={"pdf": "hist"}, kernel={"bandwidth_scale": [3]},
                                         observables=("energy",)), dump)
    assert py == cpp == [("flat", "hist", []), ("line", "kernel", [3.0])]


def test_config_without_the_keys_loads_as_before(tmp_path, dump):
    py, cpp = both(tmp_path, config_text(kernel={"pdf": None}), dump)
    assert py == cpp == [("flat", "hist", []), ("line", "hist", [])]
    w = workloads.Signal(np.zeros((3, 2), np.float32), 2, 1.0, 0)
    assert w.pdf == "hist" and w.bandwidth_scale is None


@pytest.mark.parametrize("hist,kernel,message", [
    (None, {"pdf": "kde"}, 'signal \'line\': unknown "pdf" "kde" ("hist" or "kernel")'),
    ({"bandwidth_scale": 1.0}, None, 'signal \'flat\': "bandwidth_scale" is only for "pdf": "kernel"'),
    ({"pdf": "hist", "bandwidth_scale": [1.0, 1.0]}, None,
     'signal \'flat\': "bandwidth_scale" is only for "pdf": "kernel"'),
    (None, {"bandwidth_scale": [1.0, 1.0, 1.0]}, 'signal \'line\': "bandwidth_scale" has 3 values for 2 fit observables'),
    (None, {"bandwidth_scale": []}, 'signal \'line\': "bandwidth_scale" has 0 values for 2 fit observables'),
    (None, {"bandwidth_scale": [1.0, 0.0]}, 'signal \'line\': "bandwidth_scale" must be positive and finite'),
    (None, {"bandwidth_scale": -2}, 'signal \'line\': "bandwidth_scale" must be positive and finite'),
    (None, {"bandwidth_scale": "1e999"}, None),
    (None, {"pdf": 3}, "pdf: not a string"),
    (None, {"bandwidth_scale": [1.0, "2"]}, "bandwidth_scale: not a number"),
])
def test_config_errors_have_the_same_message(tmp_path, dump, hist, kernel, message):
    text = config_text(hist=hist, kernel=kernel)
    if message is None:      # a number that overflows to infinity in both parsers
        text = text.replace('"1e999"', "1e999")
        message = 'signal \'line\': "bandwidth_scale" must be positive and finite'
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == ("error", message)


def test_build_workload_carries_pdf_and_scales(tmp_path):
    rng = np.random.default_rng(3)
    for name, n in (("flat", 500), ("line", 200)):
        io.write_table(tmp_path / (name + ".npz"), np.stack([rng.uniform(0, 10, n), rng.uniform(0, 6, n)], axis=1),
                       ["e", "r"])
    (tmp_path / "fit.json").write_text(config_text(kernel={"bandwidth_scale": [0.5, 2.0]}))
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    assert [s.pdf for s in w.signals] == ["hist", "kernel"]
    assert w.signals[0].bandwidth_scale is None and w.signals[1].bandwidth_scale == [0.5, 2.0]
    with pytest.raises(ValueError) as e:
        MCMC(w)
    assert "'line'" in str(e.value) and "C++" in str(e.value)


def test_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    assert NEW_ENTRY_POINTS <= set(declared_symbols())
    assert NEW_ENTRY_POINTS <= exported(capi.LIB_PATH)
    assert NEW_ENTRY_POINTS <= set(capi.SIGNATURES)


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    out = np.zeros(8, np.float32)
    assert lib.sxmc_kde_random_sample(None, 2, 1, None, None, capi.ptr(out)) == capi.ERR_INVALID
    assert lib.sxmc_kde_random_sample(None, 0, 1, None, None, None) == capi.ERR_INVALID
    h = C.c_void_p(0)
    assert lib.sxmc_kde_create_shared(None, C.byref(h)) == capi.ERR_INVALID and not h.value
    assert lib.sxmc_kde_create_shared(None, None) == capi.ERR_INVALID
    n = C.c_size_t(0)
    assert lib.sxmc_kde_sample_pool(None, C.byref(n)) == capi.ERR_INVALID
    assert "null" in capi.last_error()


def test_python_mcmc_refuses_a_kernel_signal_before_device_work():
    samples = np.zeros((10, 2), np.float32)
    sigs = [workloads.Signal(samples, 2, 10.0, 0), workloads.Signal(samples, 2, 5.0, 1, pdf="kernel")]
    sigs[1].name = "narrow_line"
    w = workloads.Workload("mixed", 1, [0.0], [1.0], [4], sigs, [], [], np.zeros((0, 2), np.float32), "test")
    with pytest.raises(ValueError) as e:
        MCMC(w, seed=1)
    assert "'narrow_line'" in str(e.value) and "sxmc::MCMC" in str(e.value)


def test_kde_ensemble_driver_compiles_and_needs_a_device(tmp_path):
    exe = build_cpp(tmp_path, "kde_ensemble")
    if capi.device_count() > 0:
        return   # (with a device it runs: tests/test_gpu_kde_sample.py)
    r = subprocess.run([exe, str(tmp_path / "none.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no GPU device" in r.stdout
