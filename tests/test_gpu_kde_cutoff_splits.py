"""GPU tests of the culled pair sum (sxmc_amd/csrc/kde_kernels.hip, kde_pairs_cutoff_kernel) where a workgroup walks
many tiles: the shapes of tests/test_gpu_kde_cutoff.py give every workgroup one tile, so the ballot there never has
more than one bit set and the round loop runs once.  Here, at the shapes of kde_cutoff_reference.REGIMES:
  A, A'   2 to 64 tiles to a workgroup: several set bits walked in one ballot, and a last split that holds fewer tiles
          than the others (t1 clipped to the number of tiles);
  B1, B2  more than 64 tiles, not a multiple of 64: a second round of 64 lanes whose base is not the split's first
          tile, partly filled; B2 with two such splits, the second clipped;
  C1, C2  shapes at which kde_cutoff.h's cutoff_split doubles the plain split's tiles per workgroup.
Every test reads the split the evaluator will launch with (EvalKernel.PairSplit) and asserts the property its regime is
named for; on a device with another number of compute units than 256, where a property may not hold, it skips with
the split in the message.  Values against the envelope of tests/kde_cutoff_reference.py on a strided subsample of the
caller's points (the sorted waves mix the caller's order, so the subsample lands in waves all over the grid), with the
envelope's negative control; the norm; the output outside the written slots; the visited tiles against the numpy
replay over all waves and tiles, strictly between none and all; two evaluations byte for byte; R = 15 against
R = +inf byte for byte; and the points set again on one evaluator under a cutoff -- many, few, none, more."""
import ctypes as C
import math

import numpy as np
import pytest

from sxmc_amd import capi
from tests.kde_cutoff_reference import (PARAMS, REGIMES, check_envelope, cutoff_points, cutoff_systs, cutoff_table,
                                        ref_cutoff, regime_inputs, strided)
from tests.test_gpu_kde_cutoff import check_stats, evaluator, run

pytestmark = pytest.mark.gpu

FIXED = [(name, D, 0.0) for name in ("A", "B1", "B2", "C1") for D in (1, 4)] + [("A'", 2, 0.0), ("C2", 2, 0.0)]
ADAPTIVE = [("A", 2, 0.5), ("B2", 2, 0.5)]
CASES = FIXED + ADAPTIVE


def case_id(c):
    return "%s-D%d-%s" % (c[0], c[1], "adaptive" if c[2] > 0 else "fixed")


def require(ok, what, label, plain, cut):
    """The property a regime is named for: asserted on 256 compute units, where the shapes were chosen; a skip, with
    the split, on a device where the plan comes out otherwise."""
    if ok:
        return
    msg = "%s: %s does not hold: split %s without a cutoff, %s with one" % (label, what, plain, cut)
    cus = capi.device_info()["compute_units"]
    assert cus != 256, msg
    pytest.skip(msg + " (%d compute units)" % cus)


def splits(ev, pts, R):
    """(the plain split, the split under R) of one evaluator with these points; it is left with the cutoff set."""
    ev.SetCutoff(0.0)
    ev.SetEvalPoints(pts)
    plain = ev.PairSplit()
    ev.SetCutoff(R)
    return plain, ev.PairSplit()


def check_regime(name, ntiles, plain, cut, label):
    nsplit, tps = cut
    print("%s: %d tiles, split (nsplit, tiles per split) %s without a cutoff, %s with one" % (label, ntiles, plain, cut))
    assert (nsplit - 1) * tps < ntiles <= nsplit * tps          # (every split has a tile, and every tile a split)
    if name in ("A", "A'"):
        require(2 <= tps <= 64 and nsplit > 1 and nsplit * tps > ntiles,
                "2 to 64 tiles per split and a shorter last split", label, plain, cut)
    if name in ("B1", "B2"):
        require(tps > 64 and tps % 64 != 0, "a partly filled second round of 64 tiles", label, plain, cut)
    if name == "B2":
        require(nsplit >= 2 and nsplit * tps > ntiles, "two splits, the last one shorter", label, plain, cut)
    if name in ("C1", "C2"):
        require(tps > plain[1], "tiles per split doubled by the cutoff", label, plain, cut)


def written_slots_only(raw, npts):
    assert raw.size == 5 + 3 * npts
    assert np.all(raw[:5] == 12345.0) and np.all(raw[6::3] == 12345.0) and np.all(raw[7::3] == 12345.0)


@pytest.mark.parametrize("name,D,alpha", CASES, ids=[case_id(c) for c in CASES])
def test_many_tiles_to_a_workgroup(name, D, alpha):
    """R = 3.  In the adaptive cases the local factors are an INPUT of the reference (ev.LocalFactors(), passed as
    lam=): ref_local_factors grows as rows^2 and cannot run at these sizes; that the factors are right is the job of
    tests/test_gpu_kde_adaptive.py."""
    R = 3.0
    label = case_id((name, D, alpha))
    samples, nf, lower, upper, pts = regime_inputs(name, D)
    npts, nrows = REGIMES[name]
    ntiles = -(-nrows // 256)
    scale, systs = [0.5] * D, cutoff_systs(D)
    ev = evaluator(samples, nf, D, lower, upper, scale, alpha, systs)
    plain, cut = splits(ev, pts, R)
    check_regime(name, ntiles, plain, cut, label)
    got = run(ev, D, lower, upper, pts, par_off=3, par_stride=2, pdf_off=5, pdf_stride=3, norm_off=1, repeat=2)
    assert ev.npoints == npts and ev.PairSplit() == cut
    idx = strided(npts, nrows)
    sub = pts.reshape(npts, D + 1)[idx].ravel()
    ref = ref_cutoff(samples, nf, D, lower, upper, scale, alpha, systs, PARAMS, sub, R,
                     lam=ev.LocalFactors() if alpha > 0 else None)
    assert got["norm"] == ref.norm and 0.5 * nrows < ref.norm < nrows
    written_slots_only(got["raw"], npts)
    assert np.isfinite(ref.full).sum() > 0.5 * len(idx)
    _, control = check_envelope(got["values"][idx], ref, "%s (%d of %d points)" % (label, len(idx), npts))
    assert control, label + ": the envelope misses an over-culled sum"
    # two evaluations give the same bytes, over all points
    assert got["outs"][0][0].tobytes() == got["outs"][1][0].tobytes()
    visited, possible = check_stats(ev, D, R, label)
    assert 0 < visited < possible
    ev.close()


@pytest.mark.parametrize("name,D", [("B2", 4), ("C1", 1)], ids=["B2-D4", "C1-D1"])
def test_radius_15_is_radius_infinity_byte_for_byte(name, D):
    """As in tests/test_gpu_kde_cutoff.py, at a shape with two rounds to a split and at a doubled one."""
    label = "%s D=%d" % (name, D)
    samples, nf, lower, upper, pts = regime_inputs(name, D)
    npts, nrows = REGIMES[name]
    scale, systs = [0.2] * D, cutoff_systs(D)
    ev = evaluator(samples, nf, D, lower, upper, scale, 0.0, systs)
    plain, cut = splits(ev, pts, 15.0)
    check_regime(name, -(-nrows // 256), plain, cut, label)
    a = run(ev, D, lower, upper, pts)
    va, pa = check_stats(ev, D, 15.0, label + " R=15")
    ev.SetCutoff(math.inf)
    assert ev.Cutoff() == math.inf and ev.PairSplit() == cut
    b = run(ev, D, lower, upper, pts)
    vb, pb = check_stats(ev, D, math.inf, label + " R=inf")
    assert a["values"].tobytes() == b["values"].tobytes() and a["norm"] == b["norm"]
    assert np.isfinite(a["values"]).sum() > 0.5 * npts and pa == pb and 0 < va < vb
    idx = strided(npts, nrows)
    sub = pts.reshape(npts, D + 1)[idx].ravel()
    ref = ref_cutoff(samples, nf, D, lower, upper, scale, 0.0, systs, PARAMS, sub, math.inf)
    assert b["norm"] == ref.norm
    check_envelope(b["values"][idx], ref, label + " R=inf")
    ev.close()


def test_reset_points_on_one_evaluator_under_a_cutoff():
    """The sequence of test_gpu_kde_dims.py's test_reset_points_on_one_evaluator at R = 3: many points, few (the point
    plan's grow-only wave boxes and order keep stale entries behind the live ones), none, then more than at first;
    then R = 0 and R = 3 again with the last points in place."""
    D, R, nrows = 3, 3.0, 4000
    ntiles = -(-nrows // 256)
    samples, nf, lower, upper = cutoff_table(D, nrows, np.random.default_rng(8900))
    scale, systs = [0.5] * D, cutoff_systs(D)
    ev = evaluator(samples, nf, D, lower, upper, scale, 0.0, systs, R=R)
    rng = np.random.default_rng(8901)
    kw = dict(par_off=3, par_stride=2, pdf_off=5, pdf_stride=3, norm_off=1)
    for npts in (40000, 7, 0, 60000):
        label = "re-set E=%d" % npts
        pts = cutoff_points(D, npts, rng, lower, upper) if npts else np.zeros(0, np.float32)
        got = run(ev, D, lower, upper, pts, **kw)
        print("%s: split %s" % (label, ev.PairSplit()))
        assert ev.npoints == npts
        if npts == 0:
            assert np.all(got["raw"] == 12345.0) and ev.CutoffStats() == (0, 0)
            assert check_stats(ev, D, R, label) == (0, 0)
            continue
        written_slots_only(got["raw"], npts)
        idx = strided(npts, nrows)
        sub = pts.reshape(npts, D + 1)[idx].ravel()
        ref = ref_cutoff(samples, nf, D, lower, upper, scale, 0.0, systs, PARAMS, sub, R)
        assert got["norm"] == ref.norm
        check_envelope(got["values"][idx], ref, label)
        visited, possible = check_stats(ev, D, R, label)
        assert 0 < visited <= possible
        if npts == 7:
            _, waves = ev.CutoffBoxes()
            assert waves.shape == (4, 8) and np.all(np.isfinite(waves[0, :D])) and np.all(np.isfinite(waves[0, 4:4 + D]))
            assert np.all(waves[1:, :4] == np.inf) and np.all(waves[1:, 4:] == -np.inf)
            assert possible == 1 * ntiles
        else:
            assert visited < possible
    # R = 0 with the 60000 points in place: the plain split and the plain evaluator's bytes; R = 3 again: its bytes
    cut = ev.PairSplit()
    plain = evaluator(samples, nf, D, lower, upper, scale, 0.0, systs)
    want = run(plain, D, lower, upper, pts, **kw)
    pdf = ev._keep["pdf"]
    ev.SetCutoff(0.0)
    assert ev.PairSplit() == plain.PairSplit()
    ev.EvalAsync()
    ev.EvalFinished()
    assert pdf.get().tobytes() == want["raw"].tobytes() and ev.CutoffStats() == (0, 0)
    assert pdf.get().tobytes() != got["raw"].tobytes()
    ev.SetCutoff(R)
    assert ev.PairSplit() == cut
    ev.EvalAsync()
    ev.EvalFinished()
    assert pdf.get().tobytes() == got["raw"].tobytes()
    ev.close()
    plain.close()


def test_no_split_without_points():
    x = np.linspace(0.1, 0.9, 300, dtype=np.float32)          # 2 tiles
    ev = evaluator(x, 1, 1, [0.0], [1.0], [1.0], 0.0, [])
    nsplit, tps = C.c_int(7), C.c_uint(7)
    assert capi.load().sxmc_kde_pair_split(ev.handle, C.byref(nsplit), C.byref(tps)) == capi.ERR_STATE
    assert (nsplit.value, tps.value) == (7, 7)
    with pytest.raises(capi.SxmcError):
        ev.PairSplit()
    ev.SetEvalPoints(np.array([0.5, 0.0], np.float32))
    assert ev.PairSplit() in ((1, 2), (2, 1))
    ev.close()
