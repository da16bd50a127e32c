"""CPU: sxmc_sample_multiplicities, the one implementation of the Monte Carlo sample weights' quantiser
(include/sxmc_hip.h), against its numpy restatement (tests/sample_weights_reference.py) as bytes; the same code as a
stand-alone program under ASan + UBSan on the same cases; and the noise model the quantiser is held to."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi
from tests import sample_weights_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "sample_weights_host")
TOP = 2**32 - 1

# name -> (weights, max_total, what is expected: (k, m) | a refusal's reason | None: whatever the restatement says)
CASES = {
    "empty": ([], 0, "zero total"),
    "one_row": ([0.75], 0, (24, [0.75 * 2**24])),
    "integers": ([3, 0, 5, 1, 2], 0, (24, [3 << 24, 0, 5 << 24, 1 << 24, 2 << 24])),
    "integers_that_need_a_negative_scale": ([3 * 2**31, 2**33], 2**31, (-3, [3 * 2**28, 2**30])),
    "ones_5_max_39": ([1.0] * 5, 39, (2, [4] * 5)),
    "ones_5_max_40": ([1.0] * 5, 40, (3, [8] * 5)),
    "single_half": ([0.5], 0, (24, [1 << 23])),
    "single_half_max_1": ([0.5], 1, (1, [1])),
    "ties_at_half_go_to_even": ([0.5, 1.5, 2.5], 8, (0, [0, 2, 2])),
    "ties_one_scale_up": ([0.25, 0.75, 1.25], 8, (1, [0, 2, 2])),
    "one_weight_needs_the_top": ([float(TOP)], 0, (0, [TOP])),
    "one_weight_half_above_the_top": ([float(TOP) + 0.5], 0, (-1, [2**31])),
    "tiny_and_huge_together": ([1e-12, 1e12], 0, (-8, [0, 3906250000])),
    "total_exactly_at_max": ([3.0, 5.0], 8 << 24, (24, [3 << 24, 5 << 24])),
    "total_one_above_max": ([3.0, 5.0], (8 << 24) - 1, (23, [3 << 23, 5 << 23])),
    "minus_zero_is_zero": ([-0.0, 1.0], 0, (24, [0, 1 << 24])),
    "nan": ([1.0, float("nan"), -1.0], 0, ("weight", 1)),
    "minus_one": ([1.0, 2.0, -1.0], 0, ("weight", 2)),
    "inf": ([float("inf")], 0, ("weight", 0)),
    "all_zero": ([0.0, 0.0], 0, "zero total"),
    "rounds_to_nothing": ([1e-30], 0, "zero total"),
    "beyond_every_scale": ([2.0**65], 0, "no scale"),
    "max_total_too_large": ([1.0], 2**32, "max_total"),
    "subnormal": ([5e-324, 1.0], 0, (24, [0, 1 << 24])),
    "random": (np.random.default_rng(3).lognormal(0, 2, 1000), 0, None),
    "random_capped": (np.random.default_rng(4).lognormal(0, 2, 1000), 40000, None),
}


def library(w, max_total):
    w = np.ascontiguousarray(w, np.float64).reshape(-1)
    m = np.full(w.size, 0xDEADBEEF, np.uint32)
    k, total = C.c_int(99), C.c_ulonglong(99)
    rc = capi.load().sxmc_sample_multiplicities(capi.ptr(w), w.size, max_total, capi.ptr(m), C.byref(k), C.byref(total))
    return rc, m, k.value, total.value


def restated(name):
    w, max_total, _ = CASES[name]
    try:
        return ref.sample_multiplicities(w, max_total)
    except ref.Refused as r:
        return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_equals_the_restatement(name):
    w, max_total, expected = CASES[name]
    want = restated(name)
    rc, m, k, total = library(w, max_total)
    if isinstance(want, ref.Refused):
        assert rc == capi.ERR_INVALID, (rc, capi.last_error())
        if want.why == "weight":
            assert "row %d " % want.row in capi.last_error(), capi.last_error()
        return
    assert rc == capi.OK, capi.last_error()
    assert (k, total) == want[1:] and m.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][2] is not None))
def test_the_restatement_gives_what_the_law_says(name):
    """The restatement is itself held to answers worked out by hand from the law."""
    expected = CASES[name][2]
    got = restated(name)
    if isinstance(expected, str):
        assert isinstance(got, ref.Refused) and got.why == expected
    elif isinstance(expected[0], str):
        assert isinstance(got, ref.Refused) and (got.why, got.row) == expected
    else:
        k, m = expected
        assert got[1] == k and got[0].tolist() == [int(x) for x in m] and got[2] == sum(int(x) for x in m)


@pytest.mark.parametrize("build", ["", "_asan"])
def test_stand_alone_program_plain_and_sanitized(build, tmp_path):
    """The header alone, with its own main, plain and under -fsanitize=address,undefined: every case's bytes."""
    exe = HOST + build
    assert os.access(exe, os.X_OK), exe + " is missing: __graft_entry__.build() makes it (tests/cpp/sampleweights.mk)"
    for name in sorted(CASES):
        w, max_total, _ = CASES[name]
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
        src.write_bytes(struct.pack("QQ", w.size, max_total) + w.tobytes())
        done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
        assert done.returncode == 0, (name, done.stderr)
        raw = dst.read_bytes()
        status, row, k, total = struct.unpack("qqqQ", raw[:32])
        want = restated(name)
        if isinstance(want, ref.Refused):
            assert status == {"max_total": 1, "weight": 2, "no scale": 3, "zero total": 4}[want.why], name
            assert want.row is None or row == want.row
        else:
            assert status == 0 and (k, total) == want[1:] and raw[32:] == want[0].tobytes(), name


def test_consequences_of_the_law():
    rng = np.random.default_rng(9)
    w = rng.integers(0, 1000, 500).astype(np.float64)
    rc, m, k, total = library(w, 0)
    assert rc == capi.OK and np.array_equal(m.astype(np.float64), np.ldexp(w, k)) and total == int(m.astype(np.uint64).sum())
    rc, m, k, total = library(np.ones(1000), 5000)
    assert rc == capi.OK and k == 2 and np.all(m == 4) and total == 4000


def test_noise_model():
    """10^5 lognormal(0, 1) weights at a mean multiplicity of at most 40, binned by a uniform second column into 50 bins:
    a row's rounding error is uniform in +-1/2 quantum (sd 1/sqrt(12) quanta), so a bin of n_b rows is off by about
    2^-k sqrt(n_b / 12); every bin is held to five times that."""
    rng = np.random.default_rng(1)
    w = rng.lognormal(0.0, 1.0, 100000)
    which = np.minimum((rng.random(100000) * 50).astype(np.int64), 49)
    rc, m, k, total = library(w, 40 * 100000)
    assert rc == capi.OK and total <= 40 * 100000
    quantum = 2.0 ** -k
    worst = 0.0
    for b in range(50):
        sel = which == b
        n_b = int(sel.sum())
        err = abs(float(np.sum(m[sel].astype(np.float64) * quantum - w[sel])))
        bound = 5.0 * quantum * np.sqrt(n_b / 12.0)
        worst = max(worst, err / bound)
        assert err <= bound, (b, n_b, err, bound)
    print("k = %d, total = %d, worst bin at %.2f of its bound" % (k, total, worst))
