"""Weighted Monte Carlo samples in pdfz::EvalKernel, without a device: the numpy reference (tests/kde_weighted_reference.py)
against the unweighted references it extends, the host-only bandwidth law (sxmc_kde_weighted_bandwidths and the stand-alone
program over sxmc_amd/csrc/kde_weights.h, plain and under ASan + UBSan) against its restatement bit for bit, and the
planted wrong references, each of which must fail the comparisons the GPU tests make."""
import os
import struct
import subprocess

import numpy as np
import pytest

from sxmc_amd import pdfz
from tests import kde_weighted_reference as W
from tests.kde_reference import compare, ref_kde

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTS = [os.path.join(ROOT, "tests", "cpp", name) for name in ("kde_weights_host", "kde_weights_host_asan")]
STATUS = {"too few": 1, "no freedom": 2, "no spread": 3}


def bits(a):
    return np.asarray(a, np.float64).tobytes()


# ------------------------------------------------------------------ the reference against the unweighted one
@pytest.mark.parametrize("D,N,E", W.SHAPES[:4])
def test_all_ones_is_the_unweighted_reference(D, N, E):
    c = W.case(D, N, max(E, 16))
    want = ref_kde(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, dataset=c.dataset)
    got = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points,
                             np.ones(N, np.uint32), dataset=c.dataset)
    assert got.norm == want.norm and 0 < got.norm < N          # (the systematics move rows across the edge)
    assert bits(got.h) == bits(want.h)
    assert bits(got.values) == bits(want.values)
    assert bits(got.bound) == bits(want.bound)
    assert got.c_max == want.c_max


@pytest.mark.parametrize("D,N,E", W.SHAPES[:5])
def test_small_multiplicities_are_the_repeated_table(D, N, E):
    c = W.case(D, N, max(E, 16))
    m = W.small_multiplicities(c)
    got = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m,
                             dataset=c.dataset)
    rep = W.repeated_table(c.table, c.nfields, m)
    want = W.ref_kde_weighted(rep, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points,
                              np.ones(len(rep), np.uint32), dataset=c.dataset, h=got.h)
    assert got.norm == want.norm
    live = ~np.isnan(want.values) & (want.values > 0)
    assert live.sum() >= 1
    rel = np.max(np.abs(got.values[live] - want.values[live]) / want.values[live])
    print("D=%d N=%d: worst relative difference %.3g, q'_max %.3g" % (D, N, rel, got.q_max))
    assert rel <= 1e-12
    assert np.array_equal(np.isnan(got.values), np.isnan(want.values))
    # the bandwidths of the two, each by its own law, agree to a few ulps: the repeated table's unweighted rule is the
    # weighted law with n_eff = S1 and S1 - 1 degrees of freedom -- not the same numbers, hence "handed the same h"
    assert got.q_max < W.Q_LIMIT


@pytest.mark.parametrize("D,N,E", W.SHAPES)
def test_byte_test_inputs_keep_q_below_the_limit(D, N, E):
    """The condition of the GPU byte tests (all m = 8 against unweighted), asserted on the reference: no pair's q'
    reaches Q_LIMIT, fixed and adaptive (the factors in), on every shape."""
    c = W.case(D, N, E)
    ones = np.ones(N, np.uint32)
    fixed = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, ones,
                               dataset=c.dataset)
    assert fixed.q_max < W.Q_LIMIT
    adaptive = W.ref_kde_weighted(c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, ones,
                                  dataset=c.dataset, alpha=0.5)
    print("D=%d N=%d: q'_max fixed %.3g adaptive %.3g" % (D, N, fixed.q_max, adaptive.q_max))
    assert adaptive.q_max < W.Q_LIMIT


# ------------------------------------------------------------------ the bandwidth law
def host_bandwidths(c, m):
    return pdfz.kde_weighted_bandwidths(c.table, c.nfields, c.D, c.lower, c.upper, c.scale, m)


def test_power_of_two_rescaling_gives_the_same_bytes():
    for D, N, _ in W.SHAPES[:4]:
        c = W.case(D, N, 4)
        base = host_bandwidths(c, None)
        for k in (8, 32):
            got = host_bandwidths(c, np.full(N, k, np.uint32))
            for key in ("h", "sigma", "mean"):
                assert bits(got[key]) == bits(base[key]), (D, N, k, key)
            assert got["n_eff"] == base["n_eff"] == base["s1"]
        m = W.small_multiplicities(c)
        a, b = host_bandwidths(c, m), host_bandwidths(c, 4 * m)
        for key in ("h", "sigma", "mean"):
            assert bits(a[key]) == bits(b[key]), (D, N, key)
        assert a["n_eff"] == b["n_eff"] and b["s1"] == 4 * a["s1"] and b["s2"] == 16 * a["s2"]


def test_law_against_its_restatement_bit_for_bit():
    for D, N, _ in W.SHAPES[:5]:
        c = W.case(D, N, 4)
        for m in (None, W.small_multiplicities(c), np.arange(N, dtype=np.uint32) * 977 % 81,
                  np.full(N, 2 ** 21, np.uint32)):
            got, want = host_bandwidths(c, m), W.law_bandwidths(c.table, c.nfields, D, c.lower, c.upper, c.scale, m)
            for key in ("s1", "s2", "n_eff"):
                assert got[key] == want[key], (D, N, key)
            for key in ("mean", "sigma"):
                assert bits(got[key]) == bits(want[key]), (D, N, key)
            assert np.max(np.abs(got["h"] - want["h"]) / want["h"]) <= 1e-14    # (pow may differ by an ulp)
            planted = W.law_bandwidths(c.table, c.nfields, D, c.lower, c.upper, c.scale, m, plant="n_for_neff")
            if m is not None and len(set(np.asarray(m).tolist())) > 1:
                assert np.max(np.abs(got["h"] - planted["h"]) / planted["h"]) > 1e-3


def test_large_multiplicities_need_128_bits():
    c = W.case(1, 255, 4)
    m = np.zeros(255, np.uint32)
    inside = np.flatnonzero((c.table[:, 0] >= -2) & (c.table[:, 0] < 2))
    m[inside[0]], m[inside[1]] = 2 ** 31 - 1, 2 ** 31             # S2 ~ 2^63: past 64 bits with one more such row
    got, want = host_bandwidths(c, m), W.law_bandwidths(c.table, c.nfields, 1, c.lower, c.upper, c.scale, m)
    assert got["s1"] == want["s1"] == float(2 ** 32 - 1)
    assert got["s2"] == want["s2"] == float((2 ** 31 - 1) ** 2 + 2 ** 62)
    assert bits(got["sigma"]) == bits(want["sigma"]) and got["n_eff"] == want["n_eff"]


def test_refusals_by_name():
    c = W.case(2, 255, 4)
    N = 255
    with pytest.raises(pdfz.Error, match="254 given for 255 rows"):
        host_bandwidths(c, np.ones(N - 1, np.uint32))
    with pytest.raises(pdfz.Error, match="exceeds 4294967295"):
        host_bandwidths(c, np.full(N, 2 ** 25, np.uint32))
    one = np.zeros(N, np.uint32)
    inside = np.flatnonzero(np.all((c.table[:, :2] >= -2) & (c.table[:, :2] < 2), axis=1))
    one[inside[3]] = 5
    with pytest.raises(pdfz.Error, match="at least 2 samples of multiplicity > 0 inside the domain"):
        host_bandwidths(c, one)
    with pytest.raises(pdfz.Error, match="at least 2 samples inside the domain"):
        pdfz.kde_weighted_bandwidths(c.table + 100.0, c.nfields, 2, c.lower, c.upper, c.scale, None)
    flat = c.table.copy()
    flat[:, 1] = 0.25
    with pytest.raises(pdfz.Error, match="observable 1 has no spread"):
        pdfz.kde_weighted_bandwidths(flat, c.nfields, 2, c.lower, c.upper, c.scale, np.full(N, 3, np.uint32))
    with pytest.raises(pdfz.Error, match="integers in"):
        host_bandwidths(c, np.full(N, 0.5))


# ------------------------------------------------------------------ the same header, stand-alone, plain and sanitised
def write_case(path, c, m):
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", len(c.table), c.nfields, c.D, 0 if m is None else 1))
        for a in (c.lower, c.upper, c.scale):
            f.write(np.asarray(a, np.float64).tobytes())
        f.write(np.ascontiguousarray(c.table, np.float32).tobytes())
        if m is not None:
            f.write(np.ascontiguousarray(m, np.uint32).tobytes())


def read_result(path):
    raw = open(path, "rb").read()
    status, obs, live = struct.unpack_from("<qqQ", raw, 0)
    d = np.frombuffer(raw, np.float64, 15, 24)
    return dict(status=status, observable=obs, live=live, s1=d[0], s2=d[1], n_eff=d[2], mean=d[3:7], sigma=d[7:11],
                h=d[11:15])


@pytest.mark.parametrize("host", HOSTS, ids=["plain", "asan_ubsan"])
def test_standalone_program(host, tmp_path):
    assert os.access(host, os.X_OK), "tests/cpp/kdeweights.mk builds it (build())"
    cases = []
    for D, N, _ in W.SHAPES[:4]:
        c = W.case(D, N, 4)
        cases += [(c, None), (c, W.small_multiplicities(c)), (c, np.full(N, 8, np.uint32))]
    c = W.case(1, 255, 4)
    lone = np.zeros(255, np.uint32)
    lone[np.flatnonzero((c.table[:, 0] >= -2) & (c.table[:, 0] < 2))[0]] = 7
    flat = W.case(2, 256, 4)
    flat.table[:, 0] = 1.0
    empty = W.case(1, 255, 4)
    empty.table = empty.table[:0]
    cases += [(c, lone), (flat, np.full(256, 2, np.uint32)), (empty, None), (empty, np.zeros(0, np.uint32))]
    for k, (c, m) in enumerate(cases):
        src, dst = str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))
        write_case(src, c, m)
        run = subprocess.run([host, src, dst], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        got = read_result(dst)
        try:
            want = W.law_bandwidths(c.table, c.nfields, c.D, c.lower, c.upper, c.scale, m)
        except ValueError as e:
            assert got["status"] == STATUS[str(e).rstrip(" 0123456789")], (k, str(e), got["status"])
            continue
        assert got["status"] == 0, k
        assert got["live"] == want["live"] and got["s1"] == want["s1"] and got["s2"] == want["s2"]
        assert got["n_eff"] == want["n_eff"]
        assert bits(got["mean"][:c.D]) == bits(want["mean"]) and bits(got["sigma"][:c.D]) == bits(want["sigma"])
        assert np.max(np.abs(got["h"][:c.D] - want["h"]) / want["h"]) <= 1e-14


# ------------------------------------------------------------------ the planted references
@pytest.mark.parametrize("D,N,E", [W.SHAPES[1], W.SHAPES[4]])
def test_planted_references_fail_the_value_comparison(D, N, E):
    """What the GPU test holds the device's values to -- |v - ref| <= bound -- rejects each planted reference when `v` is
    the true reference rounded to f32 (the best a device can do)."""
    c = W.case(D, N, E)
    m = W.small_multiplicities(c)
    args = (c.table, c.nfields, D, c.lower, c.upper, c.scale, c.systs, W.PARAMS, c.points, m)
    true = W.ref_kde_weighted(*args, dataset=c.dataset)
    device_like = true.values.astype(np.float32)
    assert compare(device_like, true)[0]
    for plant in W.PLANTS:
        ok, ratio, _ = compare(device_like, W.ref_kde_weighted(*args, dataset=c.dataset, plant=plant))
        print("D=%d N=%d plant %s: %.3g x the bound" % (D, N, plant, ratio))
        assert not ok, plant


def test_planted_picks_differ():
    cum = np.cumsum(np.array([3, 1, 2, 2 ** 20, 5], np.uint64))
    words = np.random.default_rng(5).integers(0, 2 ** 32, 4000, dtype=np.uint64)
    true = W.pick_places(words, cum)
    target = (words * cum[-1]) >> np.uint64(32)
    assert np.all(cum[true] > target) and np.all(np.where(true > 0, cum[true - 1], 0) <= target)
    assert np.mean(W.pick_places(words, cum, "uniform") != true) > 0.5
    # first C_j >= target differs exactly where target sits on a prefix sum: words built to land there
    edge = np.array([-((-int(t) << 32) // int(cum[-1])) for t in cum[:-1]], np.uint64)
    assert np.all(W.pick_places(edge, cum, "first_ge") == W.pick_places(edge, cum) - 1)
    # all m = 8: the unweighted pick
    n = 300
    assert np.array_equal(W.pick_places(words, np.arange(1, n + 1, dtype=np.uint64) * np.uint64(8)),
                          ((words * np.uint64(n)) >> np.uint64(32)).astype(np.int64))
    # two rows of 2^31 - 1 and 2^31: nothing wraps
    big = np.array([2 ** 31 - 1, 2 ** 32 - 1], np.uint64)
    top = np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint64)
    assert W.pick_places(top, big).tolist() == [0, 0, 1, 1]
