"""CPU: the adaptive bandwidths of pdfz::EvalKernel where no device is needed -- the configuration key
"bandwidth_sensitivity" read alike by sxmc_amd/io.py and sxmc::load_config (config.h, through a dump driver built
here) with the same messages for every refusal; the three new C ABI entry points declared, exported, in the ctypes table
and refusing bad arguments before any device work; the host arithmetic of the factors (sxmc_amd/csrc/kde_adaptive.h)
from a stand-alone program, plain and under ASan + UBSan; and self-checks of the numpy reference
(tests/kde_adaptive_reference.py) every GPU test compares with."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, io, pdfz, workloads
from tests.kde_adaptive_reference import ref_kde_adaptive, ref_local_factors, ref_pilot
from tests.kde_reference import compare, ref_kde
from tests.test_abi import declared_symbols, exported
from tests.test_kde_sample_cpu import build_cpp, config_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"sxmc_kde_create_adaptive", "sxmc_kde_sensitivity", "sxmc_kde_local_factors"}


# ------------------------------------------------------------------ the configuration key
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("signal_sensitivity_dump"), "signal_sensitivity_dump")


def both(tmp_path, text, exe):
    """(python result, C++ result): each a list of (name, pdf, bandwidth_sensitivity), or ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = [(s["name"], s["pdf"], float(s["bandwidth_sensitivity"])) for s in fc.signals]
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        cpp = [(s["name"], s["pdf"], s["bandwidth_sensitivity"]) for s in json.loads(r.stdout)["signals"]]
    else:
        assert r.returncode == 1 and r.stderr.startswith("signal_sensitivity_dump: "), r.stderr
        cpp = ("error", r.stderr[len("signal_sensitivity_dump: "):].strip())
    return py, cpp


def test_key_accepted_and_defaulted(tmp_path, dump):
    py, cpp = both(tmp_path, config_text(), dump)
    assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", 0.0)]                 # absent: fixed bandwidths
    for v in (0.5, 0, 1, 0.123456789012345):
        py, cpp = both(tmp_path, config_text(kernel={"bandwidth_sensitivity": v}), dump)
        assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", float(v))]
    py, cpp = both(tmp_path, config_text(kernel={"bandwidth_sensitivity": 0.25, "bandwidth_scale": [0.5, 2.0]}), dump)
    assert py == cpp == [("flat", "hist", 0.0), ("line", "kernel", 0.25)]


@pytest.mark.parametrize("hist,kernel,message", [
    ({"bandwidth_sensitivity": 0.5}, None, 'signal \'flat\': "bandwidth_sensitivity" is only for "pdf": "kernel"'),
    ({"pdf": "hist", "bandwidth_sensitivity": 0}, None,
     'signal \'flat\': "bandwidth_sensitivity" is only for "pdf": "kernel"'),
    (None, {"pdf": None, "bandwidth_sensitivity": 0.5},
     'signal \'line\': "bandwidth_sensitivity" is only for "pdf": "kernel"'),
    (None, {"bandwidth_sensitivity": 1.5}, 'signal \'line\': "bandwidth_sensitivity" must be a number in [0, 1]'),
    (None, {"bandwidth_sensitivity": -0.01}, 'signal \'line\': "bandwidth_sensitivity" must be a number in [0, 1]'),
    (None, {"bandwidth_sensitivity": "1e999"}, None),
    (None, {"bandwidth_sensitivity": "0.5"}, "bandwidth_sensitivity: not a number"),
    (None, {"bandwidth_sensitivity": [0.5]}, "bandwidth_sensitivity: not a number"),
])
def test_key_refused_with_the_same_message(tmp_path, dump, hist, kernel, message):
    text = config_text(hist=hist, kernel=kernel)
    if message is None:      # a number that overflows to infinity in both parsers
        text = text.replace('"1e999"', "1e999")
        message = 'signal \'line\': "bandwidth_sensitivity" must be a number in [0, 1]'
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == ("error", message)


def test_signal_pdf_keeps_its_two_values_and_the_workload_carries_the_key(tmp_path):
    assert io.signal_pdf("line", {"pdf": "kernel", "bandwidth_sensitivity": 0.5}, 2) == ("kernel", [1.0, 1.0])
    assert io.signal_sensitivity("line", {}, "kernel") == 0.0 and io.signal_sensitivity("flat", {}, "hist") == 0.0
    s = workloads.Signal(np.zeros((3, 2), np.float32), 2, 1.0, 0)
    assert s.bandwidth_sensitivity == 0.0
    rng = np.random.default_rng(3)
    for name, n in (("flat", 500), ("line", 200)):
        io.write_table(tmp_path / (name + ".npz"), np.stack([rng.uniform(0, 10, n), rng.uniform(0, 6, n)], axis=1),
                       ["e", "r"])
    (tmp_path / "fit.json").write_text(config_text(kernel={"bandwidth_sensitivity": 0.75}))
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    assert [s.bandwidth_sensitivity for s in w.signals] == [0.0, 0.75]
    (tmp_path / "fit.json").write_text(config_text())
    w = io.build_workload(io.load_config(str(tmp_path / "fit.json")))
    assert [s.bandwidth_sensitivity for s in w.signals] == [0.0, 0.0]


# ------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    assert NEW_ENTRY_POINTS <= set(declared_symbols())
    assert NEW_ENTRY_POINTS <= exported(capi.LIB_PATH)
    assert NEW_ENTRY_POINTS <= set(capi.SIGNATURES)


def test_bad_arguments_are_refused_without_a_device():
    lib = capi.load()
    x = np.linspace(0.1, 0.9, 50, dtype=np.float32)
    lo, hi, sc = np.zeros(1), np.ones(1), np.ones(1)
    for alpha in (-0.1, 1.1, math.nan, math.inf):
        h = C.c_void_p(0)
        rc = lib.sxmc_kde_create_adaptive(capi.ptr(x), x.size, 0, 1, 1, capi.ptr(lo), 1, capi.ptr(hi), 1, capi.ptr(sc),
                                          1, 0, alpha, C.byref(h))
        assert rc == capi.ERR_INVALID and not h.value
        assert capi.last_error() == "Bandwidth sensitivity must be a number in [0, 1]."
        with pytest.raises(pdfz.Error):
            pdfz.EvalKernel(x, 1, 1, [0.0], [1.0], [1.0], bandwidth_sensitivity=alpha)
    # the constructor's own checks come first at a valid sensitivity, with their messages
    h = C.c_void_p(0)
    assert lib.sxmc_kde_create_adaptive(capi.ptr(x), x.size, 0, 3, 1, capi.ptr(lo), 1, capi.ptr(hi), 1, capi.ptr(sc), 1,
                                        0, 0.5, C.byref(h)) == capi.ERR_INVALID
    assert capi.last_error() == "Length of samples array is not divisible by number of fields."
    v = C.c_double(7.0)
    assert lib.sxmc_kde_sensitivity(None, C.byref(v)) == capi.ERR_INVALID
    assert lib.sxmc_kde_local_factors(None, capi.ptr(np.zeros(4)), 4) == capi.ERR_INVALID


# ------------------------------------------------------------------ the host arithmetic
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan-ubsan"])
def test_host_arithmetic_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "kde_adaptive_host")
    src = os.path.join(ROOT, "tests", "cpp", "kde_adaptive_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, src], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "kde_adaptive_host: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the reference checks itself
def table(rng, n, D, outside=0.1):
    lower = np.array([-1.0, 0.0, 2.0, -3.0][:D])
    upper = lower + np.array([4.0, 1.5, 6.0, 2.5][:D])
    mid, wid = (lower + upper) / 2, upper - lower
    x = mid + 0.2 * wid * rng.normal(size=(n, D))
    out = rng.random(n) < outside
    x[out, 0] = upper[0] + 0.3 * rng.random(out.sum())
    # (multiples of 2^-10: a shift by an integer is exact in f32)
    return (np.round(x * 1024) / 1024).astype(np.float32), lower, upper


@pytest.mark.parametrize("D", [1, 2, 3])
def test_reference_factors(D):
    rng = np.random.default_rng(40 + D)
    x, lower, upper = table(rng, 800, D)
    args = (x.ravel(), D, D, lower, upper, [1.0] * D)
    assert np.all(ref_local_factors(*args, 0.0) == 1.0)                                   # alpha = 0: all ones
    f, inside, _ = ref_pilot(*args)
    assert 0 < (~inside).sum() < 200 and np.all(f[inside] > 0)
    lam = ref_local_factors(*args, 0.5, clip=False)
    assert abs(float(np.sum(np.log(lam[inside])))) < 1e-9 * inside.sum()                  # geometric mean 1
    clipped = ref_local_factors(*args, 0.5)
    assert np.all((clipped >= 0.1) & (clipped <= 10.0))
    if np.all((lam[inside] > 0.1) & (lam[inside] < 10)):
        assert np.array_equal(clipped[inside], lam[inside])
    # dense regions get narrow kernels: lambda falls as the pilot grows
    order = np.argsort(f[inside])
    assert np.all(np.diff(lam[inside][order]) <= 0)
    # a common shift of samples and domain (one a float represents exactly) leaves the factors alone
    shift = 8.0
    moved = ref_local_factors((x + np.float32(shift)).ravel(), D, D, lower + shift, upper + shift, [1.0] * D, 0.5)
    assert np.allclose(moved, clipped, rtol=1e-9, atol=0)


def test_reference_values_reduce_to_the_fixed_reference_and_integrate_to_one():
    rng = np.random.default_rng(50)
    x, lower, upper = table(rng, 400, 2)
    systs, params = [dict(type="shift", obs=0, pars=[0])], {0: 0.05}
    m = 120
    c = [lower[d] + (np.arange(m) + 0.5) / m * (upper[d] - lower[d]) for d in range(2)]
    grid = np.stack(np.meshgrid(*c, indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([grid, np.zeros((len(grid), 1))], axis=1).astype(np.float32).ravel()
    args = (x.ravel(), 2, 2, lower, upper, [1.5, 1.5])
    fixed = ref_kde(*args, systs, params, pts)
    zero = ref_kde_adaptive(*args, 0.0, systs, params, pts)
    assert zero.norm == fixed.norm and np.allclose(zero.values, fixed.values, rtol=1e-12, atol=0)
    adaptive = ref_kde_adaptive(*args, 1.0, systs, params, pts)
    cell = float(np.prod((upper - lower) / m))
    # (midpoint rule on kernels as narrow as h / 10 x a few: a per cent, not the kernels' precision)
    assert abs(float(adaptive.values.sum()) * cell - 1.0) < 0.02
    assert not compare(adaptive.values, fixed)[0]                                         # and it is another PDF
    for plant in ("fixed", "sensitivity", "weight", "power"):
        assert not compare(adaptive.values, ref_kde_adaptive(*args, 1.0, systs, params, pts, plant=plant))[0], plant
