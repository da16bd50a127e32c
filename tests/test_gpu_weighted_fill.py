"""GPU: the weighted histogram fill (sxmc_hist_set_sample_multiplicities, include/sxmc_hip.h) as BYTES against the
unchanged CPU oracle run on the table with row i repeated m_i times -- bins, norm and pdf values.  Integer counts and
commutative integer atomics: no tolerance anywhere in this file."""
import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, nll, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic

pytestmark = pytest.mark.gpu

LDS_MAX_BINS = 40960 - 128   # kLdsMaxBins (sxmc_amd/csrc/sxmc_host.h)

# per number of observables: (nfields, systematics, parameters).  1: one shift (decoded program, nslot = 1); 2: a
# TWO-coefficient scale + a cos-theta scale (decoded, nslot = 2); 3: scale + cos-theta scale + resolution scale against a
# truth field (decoded, nslot = 4); "c3": shift + scale + resolution scale, the one program the weighted fill has as
# straight-line code; 5: three resolution scales against three truth fields, nslot = 8 > nobs + 2 (the generic kernel).
SHAPES = {
    1: (1, [dict(type="shift", obs=0, pars=[0])], [0.07]),
    2: (2, [dict(type="scale", obs=0, pars=[0, 1]), dict(type="ctscale", obs=1, pars=[2])], [0.02, -0.03, 0.05]),
    3: (4, [dict(type="scale", obs=2, pars=[0]), dict(type="ctscale", obs=1, pars=[1]),
            dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])], [0.05, -0.01, 0.08]),
    # BASELINE config 3's program: the weighted fill's one straight-line kernel
    "c3": (4, [dict(type="shift", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
               dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])], [0.05, -0.01, 0.08]),
    5: (8, [dict(type="resolution_scale", obs=0, true_obs=5, pars=[0]), dict(type="resolution_scale", obs=1, true_obs=6, pars=[1]),
            dict(type="resolution_scale", obs=2, true_obs=7, pars=[2]), dict(type="shift", obs=4, pars=[1])], [0.1, -0.05, 0.2]),
}
NBINS = {1: [37], 2: [9, 11], 3: [5, 6, 7], "c3": [5, 6, 7], 5: [3, 4, 3, 2, 5]}
KIND = {1: "decoded+weighted", 2: "decoded+weighted", 3: "decoded+weighted", "c3": "builtin+weighted", 5: "generic+weighted"}


def make_table(rng, n, nfields):
    t = rng.uniform(-0.2, 1.2, size=(n, nfields)).astype(np.float32)
    if n >= 3:   # rows sitting on the lower and on the upper edge of observable 0
        t[0, 0], t[1, 0] = 0.0, 1.0
    return t


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Evaluator:
    """One EvalHist with its buffers bound; m = None: unweighted."""

    def __init__(self, table, nfields, nbins, systs, params, m=None, points=None, launch=None, shared_from=None):
        nobs = len(nbins)
        if shared_from is None:
            self.ev = pdfz.EvalHist(table, nfields, nobs, [0.0] * nobs, [1.0] * nobs, nbins)
            for s in systs:
                self.ev.AddSystematic(make_systematic(s))
            if m is not None:
                self.ev.SetSampleMultiplicities(m)
        else:
            self.ev = pdfz.EvalHist.Shared(shared_from.ev)
        self.npoints = 0
        if points is not None:
            self.ev.SetEvalPoints(points)
            self.npoints = len(points)
        self.out = DeviceArray(np.full(max(self.npoints, 1), 12345.0, np.float32))
        self.norm = DeviceArray.zeros(1, np.uint32)
        self.pbuf = DeviceArray(np.asarray(params, np.float64))
        self.ev.SetPDFValueBuffer(self.out)
        self.ev.SetNormalizationBuffer(self.norm)
        self.ev.SetParameterBuffer(self.pbuf)
        if launch:
            self.ev.SetLaunchConfig(*launch)

    def run(self, do_eval_pdf=True):
        self.ev.EvalAsync(do_eval_pdf)
        self.ev.EvalFinished()
        return self.result()

    def result(self):
        return dict(bins=self.ev.GetBins(), norm=int(self.norm.get()[0]), out=self.out.get())

    def close(self):
        self.ev.close()


def reference(table, nfields, nbins, systs, params, m, points=None):
    """The oracle on np.repeat(table, m, axis=0)."""
    nobs = len(nbins)
    geom = oracle.HistGeometry([0.0] * nobs, [1.0] * nobs, nbins)
    rep = np.repeat(np.asarray(table, np.float32).reshape(-1, nfields), np.asarray(m, np.int64), axis=0)
    bins, norm = oracle.bin_samples(geom, rep, nfields, systs, np.asarray(params, np.float64))
    res = dict(bins=bins, norm=norm)
    if points is not None:
        rb = oracle.set_eval_points(geom, points, 0)
        out = np.full(max(len(points), 1), 12345.0, np.float32)
        oracle.eval_pdf(rb, bins, norm, geom.bin_volume, out=out)
        res["out"] = out
    return res


def eval_points(rng, n, nobs):
    p = rng.uniform(-0.1, 1.1, size=(n, nobs + 1)).astype(np.float32)
    p[:, nobs] = 0.0
    return p


@pytest.mark.parametrize("nobs", [1, 2, 3, "c3", 5])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 255, 256, 257, 3001])
def test_bits_against_the_repeated_table(rows, nobs):
    nfields, systs, params = SHAPES[nobs]
    rng = np.random.default_rng(1000 * len(NBINS[nobs]) + rows + (7 if nobs == "c3" else 0))
    table = make_table(rng, rows, nfields)
    m = rng.integers(0, 4, size=rows).astype(np.uint32)
    points = eval_points(rng, 40, len(NBINS[nobs]))
    # (3 001 rows: 64 lanes per workgroup, the last workgroup's last unit clamped)
    e = Evaluator(table, nfields, NBINS[nobs], systs, params, m, points, launch=(64, 1) if rows == 3001 else None)
    assert e.ev.SampleTotal() == int(m.sum()) and e.ev.nsamples == rows
    assert np.array_equal(e.ev.SampleMultiplicities(), m)
    got = e.run()
    want = reference(table, nfields, NBINS[nobs], systs, params, m, points)
    info = _launch_info(e.ev)
    assert "program=" + KIND[nobs] in info and "table=rows" in info, info
    assert same_bits(got["bins"], want["bins"])
    assert got["norm"] == want["norm"]
    assert same_bits(got["out"], want["out"])
    again = e.run()   # two evaluations: the same bytes
    assert same_bits(again["bins"], got["bins"]) and again["norm"] == got["norm"] and same_bits(again["out"], got["out"])
    e.close()


def _launch_info(ev):
    import ctypes as C
    buf = C.create_string_buffer(8192)
    capi.call("sxmc_hist_launch_info", ev.handle, buf, len(buf))
    return buf.value.decode()


def test_many_stages_per_lane():
    """200 001 rows at 64 lanes and one workgroup per CU: every lane walks several stages, the last unit is clamped."""
    nfields, systs, params = SHAPES[1]
    rng = np.random.default_rng(7)
    table = make_table(rng, 200001, nfields)
    m = rng.integers(0, 4, size=200001).astype(np.uint32)
    e = Evaluator(table, nfields, NBINS[1], systs, params, m, launch=(64, 1))
    got = e.run(False)
    want = reference(table, nfields, NBINS[1], systs, params, m)
    assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"]
    e.close()


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("shape,nbins", [(2, [202, 202]), (2, [203, 202]), ("c3", [35, 34, 34]), ("c3", [35, 35, 34])],
                         ids=["decoded_in_lds", "decoded_beyond_lds", "builtin_in_lds", "builtin_beyond_lds"])
def test_histogram_in_lds_and_just_beyond(shape, nbins, with_points):
    in_lds = int(np.prod(nbins)) <= LDS_MAX_BINS
    assert in_lds == (nbins in ([202, 202], [35, 34, 34]))
    nfields, systs, params = SHAPES[shape]
    rng = np.random.default_rng(nbins[0] + nbins[1])
    table = make_table(rng, 3001, nfields)
    m = rng.integers(0, 4, size=3001).astype(np.uint32)
    points = eval_points(rng, 300, len(nbins)) if with_points else None
    e = Evaluator(table, nfields, nbins, systs, params, m, points)
    got = e.run()          # (with points: a lookup evaluation, dense flavour -- the histogram is filled too)
    want = reference(table, nfields, nbins, systs, params, m, points)
    assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"]
    if with_points:
        assert same_bits(got["out"], want["out"])
    info = _launch_info(e.ev)
    assert ("hist=lds" if in_lds else "hist=global") in info and "program=" + KIND[shape] in info, info
    e.close()


def test_edges_nan_and_the_row_past_the_end():
    """Rows on both edges, one ulp inside them, a NaN row with m = 3, and values close under the upper edge (where the
    index can come out one past the end: counted in the norm, not in a bin) -- whatever the oracle says, as bytes."""
    one = np.float32(1.0)
    xs = [0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(np.float32(0), one), -0.0, np.nan, 0.5,
          0.99999994, 0.9999999, 0.999999, np.inf, -np.inf]
    table = np.asarray(xs, np.float32).reshape(-1, 1)
    m = np.asarray([2, 3, 1, 2, 3, 3, 2, 1, 2, 3, 2, 1], np.uint32)
    for nbins, shift in (([7], 0.0), ([3], 0.0), ([10], 1e-9), ([10], -1e-9)):
        systs, params = [dict(type="shift", obs=0, pars=[0])], [shift]
        e = Evaluator(table, 1, nbins, systs, params, m)
        got = e.run(False)
        want = reference(table, 1, nbins, systs, params, m)
        assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"]
        e.close()


def test_large_multiplicities_by_linearity_and_the_cap():
    nfields, systs, params = SHAPES[3]
    rng = np.random.default_rng(11)
    table = make_table(rng, 257, nfields)
    m = rng.integers(0, 4, size=257).astype(np.uint32)
    a = Evaluator(table, nfields, NBINS[3], systs, params, m)
    b = Evaluator(table, nfields, NBINS[3], systs, params, 1000 * m)
    ra, rb = a.run(False), b.run(False)
    assert np.array_equal(rb["bins"].astype(np.uint64), 1000 * ra["bins"].astype(np.uint64))
    assert rb["norm"] == 1000 * ra["norm"]
    a.close()
    b.close()
    # the cap: three in-domain rows whose multiplicities add up to 2^32 - 1 exactly; one more is refused
    rows = np.asarray([[0.5], [0.25], [0.75]], np.float32)
    c = Evaluator(rows, 1, [4], [], [0.0], np.asarray([2**32 - 3, 1, 1], np.uint32))
    rc = c.run(False)
    assert rc["norm"] == 2**32 - 1 and rc["bins"].tolist() == [0, 1, 2**32 - 3, 1]
    c.close()
    ev = pdfz.EvalHist(rows, 1, 1, [0.0], [1.0], [4])
    with pytest.raises(pdfz.Error, match="exceeds 4294967295"):
        ev.SetSampleMultiplicities(np.asarray([2**32 - 3, 2, 1], np.uint32))
    ev.close()


@pytest.mark.parametrize("nobs", [1, 3, "c3"])
def test_all_equal_multiplicities_give_the_unweighted_pdf_values(nobs):
    nfields, systs, params = SHAPES[nobs]
    rng = np.random.default_rng(5 + len(NBINS[nobs]))
    table = make_table(rng, 3001, nfields)
    points = eval_points(rng, 200, len(NBINS[nobs]))
    w = Evaluator(table, nfields, NBINS[nobs], systs, params, np.full(3001, 8, np.uint32), points)
    u = Evaluator(table, nfields, NBINS[nobs], systs, params, None, points)
    rw, ru = w.run(), u.run()
    assert same_bits(rw["out"], ru["out"])          # the scale cancels exactly: bins and norm both carry 2^3
    assert rw["norm"] == 8 * ru["norm"] and np.array_equal(rw["bins"], 8 * ru["bins"])
    w.close()
    u.close()


def test_mixed_group_keeps_the_unweighted_members_as_they_were():
    """Weighted and unweighted members of one shape in one group, with a tiny weighted member so that a workgroup's slice
    spans members: every member's bytes, the unweighted ones equal to the group without the weighted members and planned
    in the same forms."""
    nfields, systs, params = SHAPES["c3"]
    rng = np.random.default_rng(21)
    tables = [make_table(rng, n, nfields) for n in (3001, 2000, 5, 3001, 1500)]
    mult = [rng.integers(0, 4, size=3001).astype(np.uint32), None, rng.integers(0, 4, size=5).astype(np.uint32),
            rng.integers(0, 4, size=3001).astype(np.uint32), None]
    points = eval_points(rng, 100, 3)

    def build(which):
        evs = [Evaluator(tables[i], nfields, NBINS[3], systs, params, mult[i], points) for i in which]
        g = nll.EvalGroup([e.ev for e in evs])
        g.EvalAsync(True)
        g.EvalFinished()
        first = [e.result() for e in evs]
        g.EvalAsync(False)
        g.EvalFinished()
        return evs, g, first, [e.result() for e in evs]

    evs, g, lookup, dense = build(range(5))
    info = g.LaunchInfo()
    for i in range(5):
        m = mult[i] if mult[i] is not None else np.ones(len(tables[i]), np.uint32)
        want = reference(tables[i], nfields, NBINS[3], systs, params, m, points)
        assert same_bits(dense[i]["bins"], want["bins"]) and dense[i]["norm"] == want["norm"], i
        assert same_bits(lookup[i]["out"], want["out"]) and lookup[i]["norm"] == want["norm"], i
    evs2, g2, lookup2, dense2 = build([1, 4])
    info2 = g2.LaunchInfo()
    for k, i in enumerate([1, 4]):
        assert same_bits(dense[i]["bins"], dense2[k]["bins"]) and same_bits(lookup[i]["out"], lookup2[k]["out"])
    # the unweighted members' launch: the same line (but its number) in both groups; the weighted class beside it
    strip = lambda text: sorted(line.split(": ", 1)[1] for line in text.splitlines() if line.startswith("launch"))
    unweighted = [l for l in strip(info) if "weighted" not in l]
    assert unweighted == strip(info2), (info, info2)
    assert sum("program=builtin+weighted" in l and "members=3" in l and "table=rows" in l for l in strip(info)) == 1, info
    with pytest.raises(capi.SxmcError) as err:   # one form only, and not every member is weighted: the old refusal
        g.SetFillForm(2)
    assert err.value.code == capi.ERR_INVALID
    for e in evs + evs2:
        e.close()
    g.close()
    g2.close()


def test_group_of_weighted_members_refuses_other_forms_and_counts_the_bytes():
    nfields, systs, params = SHAPES[3]
    rng = np.random.default_rng(22)
    table = make_table(rng, 1000, nfields)
    points = eval_points(rng, 50, 3)
    w = Evaluator(table, nfields, NBINS[3], systs, params, np.full(1000, 2, np.uint32), points)
    u = Evaluator(table, nfields, NBINS[3], systs, params, None, points)
    gw, gu = nll.EvalGroup([w.ev]), nll.EvalGroup([u.ev])
    for g in (gw, gu):
        g.SetPrebinning(False)
        g.SetBucketing(False)
    with pytest.raises(capi.SxmcError, match="sample multiplicities") as err:
        gw.SetFillForm(2)
    assert err.value.code == capi.ERR_STATE
    assert gw.AdaptFillForm() == (0, False)
    assert gw.LookaheadSupported() is False
    assert gw.AlgorithmicBytes()["fill_read"] == gu.AlgorithmicBytes()["fill_read"] + 4.0 * 1000    # 4 bytes per row more
    # lockstep sets and the look-ahead pass refuse by name, before they read any of their arguments' targets
    import ctypes as C
    arr = (C.c_void_p * 2)(gw._g, gw._g)
    h = C.c_void_p(0)
    capi.call("sxmc_multigroup_create", arr, 2, C.byref(h))
    dummy = DeviceArray.zeros(64, np.float64)
    args = (capi.StepArgs * 2)()
    for a in args:
        for field, ctype in capi.StepArgs._fields_:
            setattr(a, field, dummy.ptr if ctype is C.c_void_p else 1)
    step = capi.load().sxmc_multigroup_step_async(h, None, C.cast(args, C.c_void_p))
    assert step == capi.ERR_STATE and "sample multiplicities set: lockstep sets" in capi.last_error(), capi.last_error()
    look = capi.load().sxmc_multigroup_lookahead_step_async(h, None, C.cast(args, C.c_void_p), capi.ptr(dummy),
                                                            capi.ptr(dummy), None)
    assert look == capi.ERR_STATE and "sample multiplicities set: the look-ahead pass" in capi.last_error(), capi.last_error()
    capi.call("sxmc_multigroup_destroy", h)
    for x in (w, u):
        x.close()
    gw.close()
    gu.close()


def test_shared_evaluator_shares_the_multiplicities():
    nfields, systs, params = SHAPES[2]
    rng = np.random.default_rng(31)
    table = make_table(rng, 3001, nfields)
    m = rng.integers(0, 4, size=3001).astype(np.uint32)
    points = eval_points(rng, 60, 2)
    base = Evaluator(table, nfields, NBINS[2], systs, params, m, points)
    twin = Evaluator(None, nfields, NBINS[2], systs, [0.0, 0.01, -0.02], None, points, shared_from=base)
    assert twin.ev.SampleTotal() == int(m.sum()) and np.array_equal(twin.ev.SampleMultiplicities(), m)
    got = twin.run()
    want = reference(table, nfields, NBINS[2], systs, [0.0, 0.01, -0.02], m, points)
    assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"] and same_bits(got["out"], want["out"])
    got = base.run()
    want = reference(table, nfields, NBINS[2], systs, params, m, points)
    assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"] and same_bits(got["out"], want["out"])
    twin.close()
    base.close()


def test_drop_in_path_batches_weighted_and_unweighted_evaluators():
    """EvalAsync on every evaluator, then EvalFinished on every one -- twice, so that the second round goes out as the
    batch seen before (sxmc_hist_eval_async's deferred batches)."""
    nfields, systs, params = SHAPES["c3"]
    rng = np.random.default_rng(41)
    tables = [make_table(rng, n, nfields) for n in (3001, 257, 1000)]
    mult = [rng.integers(0, 4, size=3001).astype(np.uint32), None, rng.integers(0, 4, size=1000).astype(np.uint32)]
    points = eval_points(rng, 80, 3)
    evs = [Evaluator(t, nfields, NBINS[3], systs, params, m, points) for t, m in zip(tables, mult)]
    before = _deferred_stats()
    for _ in range(2):
        for e in evs:
            e.ev.EvalAsync(True)
        for e in evs:
            e.ev.EvalFinished()
    after = _deferred_stats()
    assert after[0] - before[0] == 2 and after[1] - before[1] == 6     # two launches carried six evaluations
    for e, t, m in zip(evs, tables, mult):
        want = reference(t, nfields, NBINS[3], systs, params, m if m is not None else np.ones(len(t), np.uint32), points)
        assert int(e.norm.get()[0]) == want["norm"] and same_bits(e.out.get(), want["out"])
        assert same_bits(e.ev.GetBins(), want["bins"])
    assert "weighted" in _launch_info(evs[0].ev)
    for e in evs:
        e.close()


def _deferred_stats():
    import ctypes as C
    a, b = C.c_ulonglong(0), C.c_ulonglong(0)
    capi.call("sxmc_deferred_eval_stats", C.byref(a), C.byref(b))
    return a.value, b.value


def test_setting_multiplicities_late_or_wrongly_is_refused():
    table = np.linspace(0.05, 0.95, 10, dtype=np.float32).reshape(-1, 1)
    e = Evaluator(table, 1, [4], [], [0.0], None)
    e.run(False)
    with pytest.raises(capi.SxmcError, match="before the evaluator's first evaluation") as err:
        e.ev.SetSampleMultiplicities(np.ones(10, np.uint32))
    assert err.value.code == capi.ERR_STATE
    e.close()
    ev = pdfz.EvalHist(table, 1, 1, [0.0], [1.0], [4])
    g = nll.EvalGroup([ev])      # joined a group, never evaluated
    with pytest.raises(capi.SxmcError) as err:
        ev.SetSampleMultiplicities(np.ones(10, np.uint32))
    assert err.value.code == capi.ERR_STATE
    g.close()
    ev.close()
    ev = pdfz.EvalHist(table, 1, 1, [0.0], [1.0], [4])
    with pytest.raises(pdfz.Error, match="one word per row"):
        ev.SetSampleMultiplicities(np.ones(9, np.uint32))
    assert ev.SampleTotal() == 10 and np.array_equal(ev.SampleMultiplicities(), np.ones(10, np.uint32))
    ev.close()
