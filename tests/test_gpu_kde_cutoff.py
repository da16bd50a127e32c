"""GPU tests of pdfz::EvalKernel's cutoff radius (include/sxmc_hip.h, sxmc_kde_set_cutoff) against the envelope of
tests/kde_cutoff_reference.py: with R > 0 a value lies between the contract value and the sum over the pairs certainly
below the cutoff, within the kernels' rounding bound.  Shapes: 255, 256, 257 and 1000 sample rows (around one
256-row tile, and several), 1, 63, 64, 65 and 300 points (around one wave of 64, and two workgroups) with points
outside the domain and of another data set among them, 1 to 4 observables, fixed and adaptive bandwidths, under
shift + scale (x 1.5) + resolution, so that the boxes of an evaluation are not those the order was made from.  Also:
R = 15 against R = +inf byte for byte; the visited tiles against a numpy replay of the visit test on the boxes read
back, and strictly fewer than possible on a table of separate clusters; everything the cutoff must leave alone
(norm, sampler, projection, R = 0) byte for byte; shared evaluators, caller's streams and recorded graphs."""
import math

import numpy as np
import pytest

from sxmc_amd import capi, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests.kde_adaptive_reference import ref_local_factors
from tests.kde_cutoff_reference import (PARAMS, POINTS, SIZES, check_envelope, clip_table, cutoff_points, cutoff_systs,
                                        cutoff_table, ref_cutoff, replay_visits)
from tests.test_gpu_kde import gpu_kde

pytestmark = pytest.mark.gpu

MODES = [(0.0, "fixed"), (0.5, "adaptive")]


def evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=None, dataset=0):
    ev = pdfz.EvalKernel(samples, nf, D, list(lower), list(upper), scale, dataset=dataset, bandwidth_sensitivity=alpha)
    for s in systs:
        ev.AddSystematic(make_systematic(s))
    if R is not None:
        ev.SetCutoff(R)
    return ev


def run(ev, D, lower, upper, pts, params=PARAMS, **kw):
    return gpu_kde(None, None, D, lower, upper, None, None, params, pts, ev=ev, **kw)


def check_stats(ev, D, R, label):
    """tiles_visited of the last evaluation against the numpy replay of the visit test on the boxes read back."""
    visited, possible = ev.CutoffStats()
    tiles, waves = ev.CutoffBoxes()
    live = np.isfinite(waves[:, 0])
    v = replay_visits(D, tiles, waves, R)
    assert not v[~live].any()
    assert possible == int(live.sum()) * len(tiles)
    print("%s: visited %d of %d tiles" % (label, visited, possible))
    assert visited == int(v.sum())
    return visited, possible


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_envelope(D, alpha, mode):
    controls = 0
    for N in SIZES:
        rng = np.random.default_rng(8000 + D if N == 1000 else 8100 + 10 * D + N)
        samples, nf, lower, upper = cutoff_table(D, N, rng)
        scale, systs = [0.5] * D, cutoff_systs(D)
        ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs)
        plain = evaluator(samples, nf, D, lower, upper, scale, alpha, systs)
        for E in POINTS:
            pts = cutoff_points(D, E, rng, lower, upper)
            base = run(plain, D, lower, upper, pts)
            for R in (3.0, 6.0):
                ev.SetCutoff(R)
                assert ev.Cutoff() == R
                got = run(ev, D, lower, upper, pts, par_off=3, par_stride=2, pdf_off=5, pdf_stride=3, norm_off=1,
                          repeat=2)
                ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, PARAMS, pts, R)
                assert got["norm"] == ref.norm == base["norm"]
                raw = got["raw"]
                assert np.all(raw[:5] == 12345.0) and np.all(raw[6::3] == 12345.0) and np.all(raw[7::3] == 12345.0)
                label = "D=%d %s N=%d E=%d R=%g" % (D, mode, N, E, R)
                _, control = check_envelope(got["values"], ref, label)
                if R == 3.0 and N == 1000 and E == 300:
                    assert control, label + ": the envelope misses an over-culled sum"
                    controls += 1
                # two evaluations give the same bytes
                assert got["outs"][0][0].tobytes() == got["outs"][1][0].tobytes()
                check_stats(ev, D, R, label)
        ev.close()
        plain.close()
    assert controls == 1


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_radius_15_is_radius_infinity_byte_for_byte(D, alpha, mode):
    """qcut(15) = 162 > 149: every dropped exp2 is exactly 0 in f32 (every weight is finite)."""
    rng = np.random.default_rng(8200 + D)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    scale, systs = [0.2] * D, cutoff_systs(D)
    pts = cutoff_points(D, 300, rng, lower, upper)
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=15.0)
    a = run(ev, D, lower, upper, pts)
    va, pa = check_stats(ev, D, 15.0, "D=%d %s R=15" % (D, mode))
    ev.SetCutoff(math.inf)
    assert ev.Cutoff() == math.inf
    b = run(ev, D, lower, upper, pts)
    vb, pb = check_stats(ev, D, math.inf, "D=%d %s R=inf" % (D, mode))
    assert a["values"].tobytes() == b["values"].tobytes() and a["norm"] == b["norm"]
    assert np.isfinite(a["values"]).sum() > 200 and pa == pb and va <= vb
    if D == 1 and alpha == 0.0:
        assert va < vb            # (and the identity is not one of two full sums)
    # R = +inf keeps every pair: the contract value within the plain rounding bound
    ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, PARAMS, pts, math.inf)
    check_envelope(b["values"], ref, "D=%d %s R=inf" % (D, mode))
    ev.close()


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
def test_a_table_of_separate_clusters_is_culled(alpha, mode):
    """1000 rows in three clusters 0.3 of the domain apart, bandwidths of a few thousandths of it: the sorted tiles
    hold a cluster or two each and a wave of sorted points sits in one, so at R = 3 the replay itself says that
    tiles are skipped."""
    D = 2
    rng = np.random.default_rng(8300)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    scale, systs = [0.2] * D, cutoff_systs(D)
    wid = upper - lower
    centre = lower + wid * np.array([0.2, 0.5, 0.8])[rng.integers(0, 3, 300)][:, None]
    p = np.zeros((300, D + 1))
    p[:, :D] = centre + 0.03 * wid * rng.normal(size=(300, D))
    pts = p.astype(np.float32).ravel()
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=3.0)
    got = run(ev, D, lower, upper, pts)
    visited, possible = check_stats(ev, D, 3.0, "clusters " + mode)
    assert 0 < visited < possible
    ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, PARAMS, pts, 3.0)
    _, control = check_envelope(got["values"], ref, "clusters " + mode)
    assert control
    # without a lookup nothing is visited; without a cutoff the statistics are zero
    run(ev, D, lower, upper, pts, do_eval_pdf=False)
    assert ev.CutoffStats() == (0, 0)
    ev.SetCutoff(0.0)
    run(ev, D, lower, upper, pts)
    assert ev.CutoffStats() == (0, 0)
    ev.close()


def test_the_adaptive_table_with_rows_at_both_clips():
    samples, nf, lower, upper = clip_table()
    D, scale, alpha = 2, [0.3, 0.3], 1.0
    lam = ref_local_factors(samples, nf, D, lower, upper, scale, alpha)
    assert np.mean(lam == 0.1) >= 0.01 and np.mean(lam == 10.0) >= 0.01
    systs = [dict(type="shift", obs=0, pars=[0]), dict(type="scale", obs=1, pars=[1])]
    params = {0: 0.01, 1: -0.004}
    rng = np.random.default_rng(8400)
    pts = cutoff_points(D, 300, rng, lower, upper)
    on = np.zeros((64, 3), np.float32)          # and points on the line, where 1 / lambda^2 = 100 decides
    on[:, :2] = (lower + upper) / 2 + 0.004 * (upper - lower) * rng.normal(size=(64, 2))
    pts = np.concatenate([pts, on.ravel()])
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs)
    for R in (3.0, 6.0):
        ev.SetCutoff(R)
        got = run(ev, D, lower, upper, pts, params=params)
        ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, params, pts, R)
        assert got["norm"] == ref.norm
        _, control = check_envelope(got["values"], ref, "clips R=%g" % R)
        assert control or R != 3.0
        tiles, _ = ev.CutoffBoxes()
        assert tiles[:, 8].min() < 0.02 and tiles[:, 8].min() >= 0.0099        # the smallest g of a tile: 1 / 10^2
        check_stats(ev, D, R, "clips R=%g" % R)
    ev.close()


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
def test_first_tile_outside_the_domain_and_a_table_moved_out_entirely(alpha, mode):
    D = 2
    rng = np.random.default_rng(8500)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng, first_tile_outside=True)
    x0 = samples.reshape(-1, nf)[:256, 0]
    assert np.all(x0 < lower[0])
    scale, systs = [0.5] * D, cutoff_systs(D)
    pts = cutoff_points(D, 300, rng, lower, upper)
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=3.0)
    for params in (PARAMS, {0: 0.2, 1: 0.5, 2: 0.1}):          # the larger shift moves part of that tile in
        got = run(ev, D, lower, upper, pts, params=params)
        ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, params, pts, 3.0)
        assert got["norm"] == ref.norm
        check_envelope(got["values"], ref, "first tile outside " + mode)
        check_stats(ev, D, 3.0, "first tile outside " + mode)
    # every row moved out: norm 0, NaN at the live points, 0 for the other data set, nothing visited
    out = run(ev, D, lower, upper, pts, params={0: 1000.0, 1: 0.5, 2: 0.1})
    ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, {0: 1000.0, 1: 0.5, 2: 0.1}, pts, 3.0)
    assert out["norm"] == ref.norm == 0
    v = out["values"]
    assert np.array_equal(np.isnan(v), np.isnan(ref.full)) and v[2] == 0.0 and math.isnan(v[0])
    visited, possible = check_stats(ev, D, 3.0, "moved out " + mode)
    assert visited == 0 and possible > 0
    ev.close()


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("D", [1, 3])
def test_what_the_cutoff_leaves_alone(D, alpha, mode):
    rng = np.random.default_rng(8600 + D)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    scale, systs = [0.5] * D, cutoff_systs(D)
    pts = cutoff_points(D, 300, rng, lower, upper)
    plain = evaluator(samples, nf, D, lower, upper, scale, alpha, systs)
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=6.0)
    assert plain.Cutoff() == 0.0 and plain.CutoffStats() == (0, 0)
    a, b = run(plain, D, lower, upper, pts), run(ev, D, lower, upper, pts)
    assert a["norm"] == b["norm"] and a["values"].tobytes() != b["values"].tobytes()
    assert ev.SamplePool() == plain.SamplePool() == a["norm"]
    assert ev.RandomSample(20000, 11).tobytes() == plain.RandomSample(20000, 11).tobytes()
    for obs in range(D):
        assert ev.Project(obs, 65).tobytes() == plain.Project(obs, 65).tobytes()
    assert ev.Bandwidths().tobytes() == plain.Bandwidths().tobytes()
    assert ev.LocalFactors().tobytes() == plain.LocalFactors().tobytes()
    # a shared evaluator: the same R, the same bytes -- made before or after the points, and outliving its base
    shared = pdfz.EvalKernel.Shared(ev)
    assert shared.Cutoff() == 6.0
    c = run(shared, D, lower, upper, pts)
    assert c["norm"] == b["norm"] and c["values"].tobytes() == b["values"].tobytes()
    assert shared.CutoffStats() == ev.CutoffStats() and ev.CutoffStats()[0] > 0
    # R = 0 after R = 6 gives back the R = 0 bytes, with points already set and with new ones
    ev.SetCutoff(0.0)
    ev.EvalAsync()
    ev.EvalFinished()
    assert b["ev"]._keep["pdf"].get()[:300].tobytes() == a["values"].tobytes()
    d = run(ev, D, lower, upper, pts)
    assert d["values"].tobytes() == a["values"].tobytes() and ev.CutoffStats() == (0, 0)
    # ... and R = 6 again, set with the points in place, the R = 6 bytes
    ev.SetCutoff(6.0)
    ev.EvalAsync()
    ev.EvalFinished()
    assert ev._keep["pdf"].get()[:300].tobytes() == b["values"].tobytes()
    ev.close()
    e = run(shared, D, lower, upper, pts)
    assert e["values"].tobytes() == b["values"].tobytes()
    # a cutoff first set on a shared evaluator of a base without one
    late = pdfz.EvalKernel.Shared(plain)
    assert late.Cutoff() == 0.0
    late.SetCutoff(6.0)
    f = run(late, D, lower, upper, pts)
    assert f["values"].tobytes() == b["values"].tobytes()
    assert run(plain, D, lower, upper, pts)["values"].tobytes() == a["values"].tobytes()
    for x in (plain, shared, late):
        x.close()


def test_invalid_radii_are_refused_before_any_device_work():
    lib = capi.load()
    for R in (math.nan, -1.0, 0.5, 0.999999, -math.inf):
        assert lib.sxmc_kde_set_cutoff(None, R) == capi.ERR_INVALID          # (checked before the evaluator itself)
        assert capi.last_error() == "Bandwidth cutoff must be 0 or a number >= 1 (infinity allowed)."
    x = np.linspace(0.1, 0.9, 300, dtype=np.float32)
    ev = pdfz.EvalKernel(x, 1, 1, [0.0], [1.0], [1.0])
    for R in (math.nan, 0.5, -2.0):
        with pytest.raises(pdfz.Error):
            ev.SetCutoff(R)
    assert ev.Cutoff() == 0.0
    ev.SetCutoff(1.0)
    assert ev.Cutoff() == 1.0
    with pytest.raises(pdfz.Error):
        ev.SetCutoff(math.nan)
    assert ev.Cutoff() == 1.0                                                  # a refused value changes nothing
    ev.close()


@pytest.mark.parametrize("alpha,mode", MODES, ids=[m for _, m in MODES])
def test_callers_stream_and_recorded_graph(alpha, mode):
    D = 2
    rng = np.random.default_rng(8700)
    samples, nf, lower, upper = cutoff_table(D, 1000, rng)
    scale, systs = [0.5] * D, cutoff_systs(D)
    pts = cutoff_points(D, 300, rng, lower, upper)
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs, R=4.0)
    want = run(ev, D, lower, upper, pts)
    stats = ev.CutoffStats()
    assert 0 < stats[0] <= stats[1]
    pdf, norm = ev._keep["pdf"], ev._keep["norm"]
    stream = capi.new_stream()

    def cleared():
        pdf.set(np.full(pdf.size, 12345.0, np.float32))
        norm.set(np.full(norm.size, 99, np.uint32))

    cleared()
    ev.EvalOnStream(stream)
    capi.call("sxmc_stream_synchronize", capi.ptr(stream))
    assert pdf.get()[:300].tobytes() == want["values"].tobytes() and int(norm.get()[0]) == want["norm"]
    assert ev.CutoffStats() == stats
    # a change of R while a graph is being recorded is refused; the recorded evaluation replays to the same bytes
    ev.EvalFinished()
    with capi.Graph.capture(stream) as g:
        ev.EvalOnStream(stream)
        assert capi.load().sxmc_kde_set_cutoff(ev.handle, 3.0) == capi.ERR_STATE
    for _ in range(2):
        cleared()
        g.launch(1)
        capi.call("sxmc_stream_synchronize", capi.ptr(stream))
        assert pdf.get()[:300].tobytes() == want["values"].tobytes() and int(norm.get()[0]) == want["norm"]
        assert ev.CutoffStats() == stats
    assert ev.Cutoff() == 4.0
    g.close()
    ev.close()
