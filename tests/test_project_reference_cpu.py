"""CPU: the references of the projection tests (tests/project_reference.py) checked against independent arithmetic --
the analytic kernel-density marginals against a midpoint-rule integral of the f64 pdf (tests/kde_reference.ref_kde),
the data histogram against numpy's and on planted edge values -- and the two entry points' argument checks, which
need no GPU."""

import numpy as np

from sxmc_amd import capi
from tests.kde_reference import ref_kde
from tests.project_reference import ref_data_hist, ref_kde_marginal, ref_kde_marginal_exact
from tests.test_abi import declared_symbols, exported

SYSTS = [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=0, pars=[1])]
PARAMS = np.array([0.05, -0.02])


def table(rng, D, n):
    lower = np.array([-1.0, 0.0, 2.0, -3.0][:D])
    upper = lower + np.array([4.0, 1.5, 6.0, 2.5][:D])
    x = (lower + upper) / 2 + 0.2 * (upper - lower) * rng.normal(size=(n, D))
    return x.astype(np.float32).ravel(), lower, upper


def test_marginals_sum_to_one():
    rng = np.random.default_rng(1)
    for D in (1, 2, 3, 4):
        samples, lower, upper = table(rng, D, 500)
        args = (samples, D, D, lower, upper, [1.0] * D, SYSTS, PARAMS)
        for obs in range(D):
            for nb in (1, 7, 64, 257):
                m = ref_kde_marginal(*args, obs, nb)
                e, u_max, mass_min = ref_kde_marginal_exact(*args, obs, nb)
                assert m.shape == e.shape == (nb,) and np.all(m >= 0)
                assert abs(m.sum() - 1.0) <= 1e-12 and abs(e.sum() - 1.0) <= 1e-12
                # the two differ by what rounding the rows to f32 can move, and do differ
                assert np.abs(m - e).max() <= 0.4 * u_max * 2.0 ** -24 / mass_min
        assert u_max > 1 and 0 < mass_min <= 1


def quadrature(args, D, obs, nb, m):
    """Midpoint rule over the f64 pdf: m points across every bin of `obs`, m across the whole of the other observable."""
    samples, nf, _, lower, upper = args[:5]
    w_bin = (upper[obs] - lower[obs]) / nb
    a = lower[obs] + (np.arange(nb * m) + 0.5) * (w_bin / m)
    if D == 1:
        pts = np.stack([a, np.zeros_like(a)], axis=1)
        area, per_bin = w_bin, m
    else:
        other = 1 - obs
        w_other = upper[other] - lower[other]
        b = lower[other] + (np.arange(m) + 0.5) * (w_other / m)
        grid = np.zeros((nb * m, m, 3))
        grid[:, :, obs] = a[:, None]
        grid[:, :, other] = b[None, :]
        pts = grid.reshape(-1, 3)
        area, per_bin = w_bin * w_other, m * m
    # (float32 points, as evaluators take them: the grid moves by 1e-7 of itself, far below the quadrature's error)
    v = ref_kde(*args, pts.astype(np.float32).ravel()).values
    return v.reshape(nb, per_bin).mean(axis=1) * area


def test_marginals_are_the_integral_of_the_pdf():
    rng = np.random.default_rng(2)
    for D, n, m in ((1, 200, 64), (2, 150, 24)):
        samples, lower, upper = table(rng, D, n)
        args = (samples, D, D, lower, upper, [1.0] * D, SYSTS, PARAMS)
        for obs in range(D):
            nb = 6
            exact = ref_kde_marginal_exact(*args, obs, nb)[0]
            coarse, fine = quadrature(args, D, obs, nb, m), quadrature(args, D, obs, nb, 2 * m)
            # the quadrature's own error, estimated by halving the grid once (the worst bin's)
            own = float(np.abs(fine - coarse).max())
            err = float(np.abs(fine - exact).max())
            print("D=%d obs %d: |quadrature - analytic| %.3g, the quadrature's own error %.3g" % (D, obs, err, own))
            assert 0 < own < 1e-3 and err <= own
            # a marginal with the bandwidth 1 % off is further away than that
            u_off = ref_kde_marginal(*args, obs, nb, bandwidth_factor=1.01)
            assert np.abs(fine - u_off).max() > own


def test_data_histogram_follows_tfill():
    rng = np.random.default_rng(3)
    lower, upper, bins = -1.5, 4.5, 12
    width = (upper - lower) / bins
    # away from the edges: numpy's histogram
    k = rng.integers(0, bins, 4000)
    x = (lower + (k + rng.uniform(0.05, 0.95, 4000)) * width).astype(np.float32)
    x = np.concatenate([x, np.float32([-7.0, 9.0, np.nan, -np.inf, np.inf])])
    assert np.array_equal(ref_data_hist(x, lower, upper, bins), np.histogram(x[:4000], bins, (lower, upper))[0])
    # planted: lower is counted (first bin), upper is not (np.histogram would count it), the float below upper is in the
    # last bin, an inner edge belongs to the bin it opens
    below = np.nextafter(np.float32(upper), np.float32(-np.inf))
    got = ref_data_hist(np.float32([lower, upper, below, lower + 3 * width]), lower, upper, bins)
    want = np.zeros(bins, np.int64)
    want[0] += 1
    want[int(bins * (float(below) - lower) / (upper - lower))] += 1
    want[3] += 1
    assert np.array_equal(got, want) and got[bins - 1] == 1 and got.sum() == 3
    # where the quotient of the float just below upper rounds up to `bins`, it is ROOT's overflow: not counted
    lo2, up2, b2 = 0.0, 3.0, 3
    x2 = np.nextafter(np.float32(up2), np.float32(0))
    j = int(b2 * (float(x2) - lo2) / (up2 - lo2))
    assert ref_data_hist(np.float32([x2]), lo2, up2, b2).sum() == (1 if j < b2 else 0)
    # and the product's own vectorised form agrees on all of it
    from sxmc_amd.ensemble import data_histogram
    for xs, a, b, n in ((x, lower, upper, bins), (np.float32([lower, upper, below]), lower, upper, bins),
                        (np.float32([x2]), lo2, up2, b2)):
        assert np.array_equal(data_histogram(xs, a, b, n), ref_data_hist(xs, a, b, n))


def test_entry_points_are_declared_exported_and_check_their_arguments():
    names = {"sxmc_hist_project", "sxmc_kde_project"}
    assert names <= set(declared_symbols()) and names <= set(capi.SIGNATURES)
    assert names <= exported(capi.LIB_PATH) and names <= exported(capi.MEASURE_LIB_PATH)
    lib = capi.load()
    counts, prob = np.zeros(4, np.uint64), np.zeros(4)
    # null arguments: refused before anything touches a device
    assert lib.sxmc_hist_project(None, 0, capi.ptr(counts), 4) == capi.ERR_INVALID
    assert "null" in capi.last_error()
    assert lib.sxmc_kde_project(None, 0, 4, capi.ptr(prob)) == capi.ERR_INVALID
    assert "null" in capi.last_error()
    if capi.device_count() < 1:
        return   # (an evaluator to be wrong about needs a device: tests/test_gpu_project.py has the rest, too)
    from sxmc_amd import pdfz
    x = np.linspace(0.05, 0.95, 40, dtype=np.float32)
    hist = pdfz.EvalHist(x, 1, 1, [0.0], [1.0], [4])
    kde = pdfz.EvalKernel(x, 1, 1, [0.0], [1.0], [1.0])
    assert lib.sxmc_hist_project(hist.handle, 0, None, 4) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(hist.handle, 1, capi.ptr(counts), 4) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(hist.handle, -1, capi.ptr(counts), 4) == capi.ERR_INVALID
    assert lib.sxmc_hist_project(hist.handle, 0, capi.ptr(counts), 5) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(kde.handle, 0, 4, None) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(kde.handle, 1, 4, capi.ptr(prob)) == capi.ERR_INVALID
    assert lib.sxmc_kde_project(kde.handle, 0, 0, capi.ptr(prob)) == capi.ERR_INVALID
    hist.close()
    kde.close()


def test_fit_spectra_program_compiles_and_needs_a_device(tmp_path):
    """tests/cpp/test_fit_spectra.cpp (sxmc::fit_spectra + write_fit_spectra over the C++ headers) compiles with the C++
    tests' flags; without a device it says so (with one it runs in tests/test_gpu_fit_spectra.py)."""
    import os
    import subprocess

    from tests.test_kde_cpu import ROOT, cpp_flags
    cxx, ld = cpp_flags()
    exe = str(tmp_path / "test_fit_spectra")
    src = os.path.join(ROOT, "tests", "cpp", "test_fit_spectra.cpp")
    subprocess.run(["g++"] + cxx + ["-o", exe, src] + ld, check=True, capture_output=True, text=True, timeout=600)
    if capi.device_count() > 0:
        return
    r = subprocess.run([exe, str(tmp_path), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "no GPU device" in r.stdout, r.stdout + r.stderr
    assert not (tmp_path / "out").exists()
