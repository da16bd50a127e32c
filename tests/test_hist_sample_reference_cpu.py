"""CPU: the numpy replica of the histogram event sampler (tests/hist_sample_reference.py), the law checks that the GPU
tests run on the device's events, and whether those checks can see a wrong sampler.

* The vectorised Philox equals tests/helpers.philox4x32_10 word for word.
* The replica's events pass every law check (hist_sample_reference.law_report) on known histograms.
* Negative controls: the same checks FAIL on the replica made wrong one way at a time -- `cdf >= target`, the first
  observable fastest in the unravel, the bin word reused for a coordinate, cuts applied by clamping, the float step left
  out in a domain far from zero.
* Every event of every geometry of the GPU tests keeps its bin under the evaluator's look-up, and no bin of them is
  without a float32 (share 0).
* The host samplers keep their bins too: ensemble.random_sample, and sxmc::random_sample through
  tests/cpp/hist_sample_dump --host; sxmc::sample_float, which is the kernel's float step statement for statement,
  equals the replica's bit for bit (--float).

The device stream is bit-identical to the replica (tests/test_gpu_hist_sample.py asserts it), so every statistical
assertion of the GPU tests is decided here, without a GPU, with the same cases and seeds (LAW_CASES, CUTS_*, the shape
cases): all of them were run here and pass (test_law_of_every_gpu_case_decided_here and test_law_of_the_shapes print
each p-value; the smallest of them is 0.015 against the bound 1e-4), and the attempt counts the GPU test relies on
(some event needs at least 100 attempts under the 1/500 cuts and none is exhausted; the larger call under the same cuts
exhausts some) are asserted here as well."""
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import ensemble
from tests import hist_sample_reference as R
from tests.helpers import philox4x32_10


def test_vector_philox_equals_the_scalar_one():
    rng = np.random.default_rng(1)
    e = np.concatenate([[0, 1, 255, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], rng.integers(0, 2 ** 62, 200)])
    e = e.astype(np.uint64)
    t = np.concatenate([[0, 1, 1023, 7, 0, 5], rng.integers(0, 1024, 200)]).astype(np.uint64)
    for seed in R.SEEDS + (2 ** 64 - 1,):
        w = R.words(e, t, seed)
        for i in range(e.size):
            want = philox4x32_10((int(e[i]) & 0xFFFFFFFF, int(e[i]) >> 32, int(t[i]), 0),
                                 (seed & 0xFFFFFFFF, seed >> 32))
            assert tuple(int(x[i]) for x in w) == want
    # Random123's known answer for the all-zero counter and key
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert tuple(int(x) for x in R.philox4x32_10_np((0, 0, 0, 0), (0, 0))) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C,
                                                                                0x9B00DBD8)


def report(case, bins, n, seed, cuts=None, variant=None):
    lo, hi = cuts if cuts else (None, None)
    d = R.draw(bins, case.geom, n, seed, lo, hi, variant=variant)
    assert d["exhausted"] == 0
    return d, R.law_report(d["events"], R.lookup(d["events"], case.geom), bins, case.geom, lo, hi)


def test_hand_made_histograms():
    g = R.Geometry([0.0, 10.0], [1.0, 13.0], [2, 3])
    bins = np.array([0, 3, 0, 2, 0, 5], np.uint32)                      # cdf 0 3 3 5 5 10
    d = R.draw(bins, g, 100000, 4)
    counts = np.bincount(d["flat"], minlength=6)
    assert np.all(counts[bins == 0] == 0)
    assert np.all(np.abs(counts - 1e4 * bins) < 5 * np.sqrt(1e4 * bins * (1 - bins / 10.0) + 1))
    assert np.array_equal(R.lookup(d["events"], g), d["flat"]) and np.all(d["attempts"] == 1)
    # the words in the order y, z: recomputed by hand for one event
    w = philox4x32_10((77, 0, 0, 0), (4, 0))
    flat = int(np.searchsorted(np.cumsum(bins), (w[0] * 10) >> 32, side="right"))
    want = [0.0 + (flat // 3 + (w[1] + 0.5) / 2 ** 32) * 0.5, 10.0 + (flat % 3 + (w[2] + 0.5) / 2 ** 32) * 1.0]
    assert d["flat"][77] == flat and np.array_equal(d["events"][77, :2], np.asarray(want, np.float32))
    one = R.draw(np.array([0, 0, 0, 0, 7, 0], np.uint32), g, 1000, 5)
    assert np.all(one["flat"] == 4)


@pytest.mark.parametrize("name", sorted(R.LAW_CASES))
def test_law_of_every_gpu_case_decided_here(name):
    make, n, seed, cuts = R.LAW_CASES[name]
    case = make()
    d, rep = report(case, case.oracle_bins(), n, seed, cuts)
    assert all(rep.values()), rep
    assert np.array_equal(R.lookup(d["events"], case.geom), d["flat"])


def test_two_seeds_share_no_row():
    case = R.case_3d()
    bins = case.oracle_bins()
    a = R.draw(bins, case.geom, R.LAW_CASES["3d"][1], R.LAW_CASES["3d"][2])["events"]
    b = R.draw(bins, case.geom, R.LAW_CASES["3d_other_seed"][1], R.LAW_CASES["3d_other_seed"][2])["events"]
    assert R.rows_in_common(a, b, 3) == 0


@pytest.mark.parametrize("case", R.shape_cases(), ids=lambda c: c.name)
def test_law_of_the_shapes(case):
    bins = case.oracle_bins()
    d, rep = report(case, bins, 100000, 21)
    rep.pop("unique", None)          # (one bin of a few floats per axis: rows do repeat)
    assert all(rep.values()), rep
    assert np.all(bins[d["flat"]] > 0)


def test_attempt_counts_under_narrow_cuts():
    case = R.case_3d()
    bins = case.oracle_bins()
    lo, hi, n, seed = R.CUTS_3D["one_in_500"]
    d = R.draw(bins, case.geom, n, seed, lo, hi)
    print("1/500 cuts: attempts", d["attempts"])
    assert d["exhausted"] == 0 and d["attempts"].max() >= 100
    lo, hi, n, seed = R.CUTS_3D["one_in_500_fails"]
    d = R.draw(bins, case.geom, n, seed, lo, hi)
    print("1/500 cuts, %d events: %d exhausted" % (n, d["exhausted"]))
    assert 0 < d["exhausted"] < n
    lo, hi, n, seed = R.CUTS_3D["one_in_sixty"]
    d = R.draw(bins, case.geom, n, seed, lo, hi)
    assert d["exhausted"] == 0 and d["attempts"].max() >= 300
    for cuts, make in ((R.CUTS_1D["one_bin"], R.case_1d), (R.CUTS_2D["one_bin"], R.case_2d)):
        c = make()
        lo, hi, n, seed = cuts
        d = R.draw(c.oracle_bins(), c.geom, n, seed, lo, hi)
        assert d["exhausted"] == 0 and np.unique(d["flat"]).size == 1


# ------------------------------------------------------------------------------------ negative controls
def failures(rep):
    return sorted(k for k, v in rep.items() if not v)


def test_control_cdf_greater_or_equal_is_seen():
    case = [c for c in R.shape_cases() if c.name == "mostly_empty"][0]
    _, rep = report(case, case.oracle_bins(), 100000, 21, variant="ge")
    print(failures(rep))
    assert "bins" in failures(rep) or "empty" in failures(rep)


def test_control_first_observable_fastest_is_seen():
    for make, key in ((R.case_2d, "2d"), (R.case_3d, "3d")):
        case = make()
        _, n, seed, _ = R.LAW_CASES[key]
        _, rep = report(case, case.oracle_bins(), n, seed, variant="first_fastest")
        print(failures(rep))
        assert "bins" in failures(rep)


def test_control_reused_bin_word_is_seen():
    for key in ("1d", "2d", "3d"):
        make, n, seed, _ = R.LAW_CASES[key]
        case = make()
        _, rep = report(case, case.oracle_bins(), n, seed, variant="reuse_word")
        print(failures(rep))
        assert "perbin_0" in failures(rep)


def test_control_reused_coordinate_word_is_seen_by_the_joint_cells():
    """(what the joint sub-cells are for: observable 1 built from observable 0's word)"""
    make, n, seed, _ = R.LAW_CASES["2d"]
    case = make()
    bins = case.oracle_bins()
    d = R.draw(bins, case.geom, n, seed)
    ev = d["events"].copy()
    g = case.geom
    f0 = (ev[:, 0].astype(np.float64) - g.lower[0]) * g.scale[0] % 1.0
    i1 = (d["flat"] // g.stride[1]) % g.nbins[1]
    ev[:, 1] = (g.lower[1] + (i1 + f0) * g.width[1]).astype(np.float32)
    rep = R.law_report(ev, R.lookup(ev, g), bins, g)
    print(failures(rep))
    assert "joint" in failures(rep) and "inside_1" not in failures(rep)


def test_control_clamped_cuts_are_seen():
    for key in ("1d_cuts", "3d_cuts"):
        make, n, seed, cuts = R.LAW_CASES[key]
        case = make()
        _, rep = report(case, case.oracle_bins(), n, seed, cuts, variant="clamp_cuts")
        print(failures(rep))
        assert "bins" in failures(rep) and "inside_0" in failures(rep)


@pytest.mark.parametrize("name", sorted(R.FAR))
def test_control_missing_float_step_is_seen_and_the_float_step_keeps_every_bin(name):
    case = R.far_case(name)
    bins = case.oracle_bins()
    old = R.draw(bins, case.geom, R.FAR_EVENTS, R.FAR_SEED, variant="no_float_step")
    rb = R.lookup(old["events"], case.geom)
    hops, outside = int(((rb != old["flat"]) & (rb >= 0)).sum()), int((rb < 0).sum())
    print("%s without the float step: %d of %d events in another bin, %d outside the domain"
          % (name, hops, R.FAR_EVENTS, outside))
    assert hops > 0 and outside > 0
    new = R.draw(bins, case.geom, R.FAR_EVENTS, R.FAR_SEED)
    rb = R.lookup(new["events"], case.geom)
    assert np.array_equal(rb, new["flat"]) and np.all(bins[rb] > 0)
    assert new["nofloat"].sum() == 0                       # the share of bins without a float32: 0
    # the float step moves a float by one place at most, and only the floats that had left
    moved = old["events"][:, 0] != new["events"][:, 0]
    assert moved.sum() == hops + outside
    assert np.all(np.abs(old["events"][moved, 0].view(np.int32).astype(np.int64) -
                         new["events"][moved, 0].view(np.int32).astype(np.int64)) == 1)


def test_every_geometry_of_the_gpu_tests_has_a_float_in_every_bin():
    cases = [R.case_1d(1000), R.case_2d(1000), R.case_3d(1000)] + R.shape_cases() + [R.far_case(k, 1000) for k in R.FAR]
    for c in cases:
        g = c.geom
        for k in range(g.nobs):
            idx = np.arange(g.nbins[k])
            mid = g.lower[k] + (idx + 0.5) * g.width[k]
            xf, nofloat = R.settle(mid, idx, g, k)
            assert not nofloat.any() and np.array_equal(R.lookup_axis(xf, g, k), idx), c.name


def test_a_bin_without_a_float_gets_the_nearest_in_domain_float():
    g = R.Geometry([1e6], [1e6 + 1], [64])                 # bins of 1/64 where floats are 1/16 apart
    bins = np.ones(64, np.uint32)
    d = R.draw(bins, g, 20000, 3)
    x = d["events"][:, 0].astype(np.float64)
    assert d["nofloat"].mean() > 0.5 and np.all((x >= 1e6) & (x < 1e6 + 1))
    kept = ~d["nofloat"]
    assert np.array_equal(R.lookup(d["events"], g)[kept], d["flat"][kept])
    xd = 1e6 + (d["flat"] + 0.5) / 64.0
    assert np.all(np.abs(x - xd) <= 1 / 16.0)


# ------------------------------------------------------------------------------------ the host samplers
@pytest.mark.parametrize("name", sorted(R.FAR))
def test_host_sampler_keeps_its_bins_far_from_zero(name):
    lo, hi, nb = R.FAR[name]
    g = R.Geometry([lo, 0.0], [hi, 1.0], [nb, 3])
    rng = np.random.default_rng(6)
    bins = rng.integers(0, 4, g.total_nbins).astype(np.uint32)
    pts = ensemble.random_sample(np.random.default_rng(7), bins, g.lower, g.upper, g.nbins, 300000)
    rb = R.lookup(pts, g)
    assert pts.dtype == np.float32 and np.all(rb >= 0) and np.all(bins[rb] > 0)
    # bit for bit what the replica's float step makes of the same f64 points
    r2 = np.random.default_rng(7)
    cdf = np.cumsum(bins, dtype=np.float64) / float(bins.sum())
    flat = np.minimum(np.searchsorted(cdf, r2.random(300000), side="right"), bins.size - 1)
    u = r2.random((300000, 2))
    assert np.array_equal(rb, flat)
    for k in range(2):
        idx = (flat // g.stride[k]) % g.nbins[k]
        want, _ = R.settle(g.lower[k] + (idx + u[:, k]) * g.width[k], idx, g, k)
        assert np.array_equal(pts[:, k], want)


@pytest.mark.parametrize("name", sorted(R.FAR))
def test_cpp_host_sampler_keeps_its_bins_far_from_zero(name, tmp_path):
    """sxmc::random_sample (ensemble.h) through tests/cpp/hist_sample_dump --host: bin i holds i % 3 counts."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "hist_sample_dump")
    lo, hi, nb = R.FAR[name]
    out = str(tmp_path / "events.f32")
    subprocess.run([exe, "--host", repr(lo), repr(hi), str(nb), "5", "300000", out], check=True, timeout=120)
    ev = np.fromfile(out, np.float32).reshape(-1, 2)
    g = R.Geometry([lo], [hi], [nb])
    rb = R.lookup(ev, g)
    assert ev.shape[0] == 300000 and np.all(ev[:, 1] == 0)
    assert np.all(rb >= 0) and np.all(rb % 3 > 0)
    counts = np.bincount(rb, minlength=nb).astype(np.float64)
    expect = 300000 * (np.arange(nb) % 3) / float((np.arange(nb) % 3).sum())
    p, _, _, _ = R.chi2_p(counts, expect)
    assert p > R.P_MIN


@pytest.mark.parametrize("lo,hi,nb", list(R.FAR.values()) + [(0.0, 10.0, 20), (0.1, 0.2, 7), (1e6, 1e6 + 1, 64)])
def test_cpp_float_step_equals_the_replicas(lo, hi, nb, tmp_path):
    """sxmc::sample_float (ensemble.h: the kernel's float step, statement for statement) against settle(), bit for
    bit, bins without a float32 included."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "hist_sample_dump")
    n = 400000
    out = str(tmp_path / "floats.f32")
    subprocess.run([exe, "--float", repr(lo), repr(hi), str(nb), str(n), out], check=True, timeout=120)
    got = np.fromfile(out, np.float32)
    g = R.Geometry([lo], [hi], [nb])
    i = np.arange(n, dtype=np.uint64)
    idx = (i % np.uint64(nb)).astype(np.int64)
    u = (((i * np.uint64(2654435761)) & R.U32).astype(np.float64) + 0.5) * 2.3283064365386963e-10
    want, nofloat = R.settle(g.lower[0] + (idx + u) * g.width[0], idx, g, 0)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(R.lookup_axis(got, g, 0)[~nofloat], idx[~nofloat])
    assert nofloat.any() == (nb == 64)
