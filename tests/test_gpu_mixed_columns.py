"""GPU: the event sum of a MIXED fit (sxmc_group_eval_columns_nll_async, columns_kernels.hip) against
nll_event_chunks over the fully materialised table, through ctypes.  The contract is bit equality: the partial sums are
compared as 64-bit integers, lane by lane, over buffers pre-filled with one sentinel (a lane that must not store shows
the sentinel in both).  Per case: the histogram members' columns of the lookup table are not written and the dense
columns are not changed; after sxmc_group_finish_columns_step_async a second step at the next proposal matches again
(the members' histograms and normalisation slots were cleared, the zero launch is skipped) and the kernel-density
members' normalisation slots survived the finish."""
import ctypes as C

import numpy as np
import pytest

from sxmc_amd import capi, nll, pdfz

pytestmark = pytest.mark.gpu

GRID, BLOCK = 64, 256
SENTINEL = np.array([0x7FF0DEADBEEF1234], np.uint64).view(np.float64)[0]   # (a NaN no lane sum can be)
LUT_SENTINEL = np.float32(-12345.5)


class Fit:
    """Evaluators (kind 'h' / 'k' per signal, in signal order), their group and the arrays of a walk over them."""

    def __init__(self, kinds, tables, nfields, nobs, lower, upper, nbins, systematics, events, syst_values,
                 member_systematics=None, seed=3):
        self.kinds, self.S = kinds, len(kinds)
        self.E = len(events)
        self.stream = capi.new_stream(nonblocking=False)
        S, E = self.S, self.E
        self.npars = S + len(syst_values)
        self.pars = capi.DeviceArray(np.concatenate([np.linspace(0.9, 1.2, S), np.asarray(syst_values, np.float64)]))
        self.lut = capi.DeviceArray(np.full(max(S * E, 1), LUT_SENTINEL, np.float32))
        self.norms = capi.DeviceArray.zeros(S, np.uint32)
        self.nexpected = capi.DeviceArray(np.linspace(40.0, 90.0, S))
        self.n_mc = capi.DeviceArray(np.array([len(t) for t in tables], np.uint32))
        self.source_id = capi.DeviceArray(np.arange(S, dtype=np.int16))
        self.evals, hists, cols = [], [], []
        for j, kind in enumerate(kinds):
            if kind == "h":
                e = pdfz.EvalHist(tables[j].ravel(), nfields, nobs, lower, upper, nbins)
                cols.append(len(hists))
                hists.append(e)
            else:
                e = pdfz.EvalKernel(tables[j].ravel(), nfields, nobs, lower, upper, [1.0] * nobs)
                cols.append(-1)
            for s in (systematics if member_systematics is None else member_systematics[j]):
                e.AddSystematic(s)
            e.SetEvalPoints(events)
            e.SetPDFValueBuffer(self.lut, j * E, 1)
            e.SetNormalizationBuffer(self.norms, j)
            e.SetParameterBuffer(self.pars, S)
            self.evals.append(e)
        self.kernels = [e for e, k in zip(self.evals, kinds) if k == "k"]
        self.hist_cols = [j for j, k in enumerate(kinds) if k == "h"]
        self.dense_cols = [j for j, k in enumerate(kinds) if k == "k"]
        self.group = nll.EvalGroup(hists)
        self.group.SetColumns(cols)
        # the rest of a step's state
        self.means = capi.DeviceArray(self.pars.get())
        self.sigmas = capi.DeviceArray(np.zeros(self.npars))
        self.rng = nll.make_rngs(self.npars, seed, self.stream)
        self.nll_current = capi.DeviceArray(np.array([1e30]))          # (the first proposal is accepted)
        self.nll_proposed = capi.DeviceArray(np.zeros(1))
        self.v_current = capi.DeviceArray(self.pars.get())
        self.accepted = capi.DeviceArray.zeros(1, np.int32)
        self.counter = capi.DeviceArray.zeros(1, np.int32)
        self.jump_buffer = capi.DeviceArray.zeros(8 * (self.npars + 1), np.float32)
        width = np.full(self.npars, 0.01, np.float32)
        self.jump_width = capi.DeviceArray(width)

    def sync(self):
        capi.call("sxmc_stream_synchronize", capi.ptr(self.stream))

    def materialised_sums(self):
        """EvalGroup.EvalAsync + the kernel evaluators' EvalAsync, then nll_event_chunks(64, 256)."""
        self.sync()
        self.group.EvalAsync(True, self.stream)
        for k in self.kernels:
            k.EvalAsync()
        for k in self.kernels:
            k.EvalFinished()
        sums = capi.DeviceArray(np.full(GRID * BLOCK, SENTINEL))
        nll.nll_event_chunks(GRID, BLOCK, self.stream, self.lut, self.pars, self.E, self.S, self.nexpected, self.n_mc,
                             self.source_id, self.norms, sums)
        self.sync()
        return sums.get().view(np.uint64), self.lut.get()[:self.S * self.E].reshape(self.S, self.E), self.norms.get()

    def in_place_sums(self, evaluate_kernels):
        if evaluate_kernels:
            for k in self.kernels:
                k.EvalOnStream(self.stream)
        sums = capi.DeviceArray(np.full(GRID * BLOCK, SENTINEL))
        self.group.EvalColumnsNllAsync(self.stream, self.lut, self.E, self.pars, self.nexpected, self.n_mc,
                                       self.source_id, self.norms, sums, GRID, BLOCK)
        self.sync()
        return sums, self.lut.get()[:self.S * self.E].reshape(self.S, self.E), self.norms.get()

    def finish(self, sums):
        self.group.FinishColumnsStepAsync(self.stream, GRID * BLOCK, sums, self.means, self.sigmas, self.rng,
                                          self.nll_current, self.nll_proposed, self.v_current, self.pars, self.accepted,
                                          self.counter, self.jump_buffer, self.npars, self.S, self.jump_width,
                                          self.nexpected, self.n_mc, self.source_id, self.norms)
        self.sync()

    def close(self):
        self.sync()
        self.group.close()
        for e in self.evals:
            e.close()


def check(fit, expect_log_free_lanes=False):
    E, S = fit.E, fit.S
    want, table, norms = fit.materialised_sums()
    # step 1: the kernel columns are in the table; the members' columns get a sentinel the entry must leave alone
    marked = table.copy()
    marked[fit.hist_cols] = LUT_SENTINEL
    if S * E:
        fit.lut.set(marked.ravel() if S * E == fit.lut.size else np.concatenate([marked.ravel(), [LUT_SENTINEL]]))
    sums, after, norms_b = fit.in_place_sums(evaluate_kernels=False)
    got = sums.get().view(np.uint64)
    print("step 1: %d lanes, %d differ; norms %s" % (got.size, int(np.sum(got != want)), list(norms_b)))
    assert np.array_equal(got, want)
    assert np.array_equal(after.view(np.uint32), marked.view(np.uint32))      # members' columns untouched, dense unchanged
    assert np.array_equal(norms_b, norms)
    untouched = int(np.sum(want == np.array([SENTINEL]).view(np.uint64)[0]))
    assert untouched == 0       # every lane stores (a lane without events stores 0.0); NaN sums do not occur here
    if expect_log_free_lanes and E:
        assert np.any(want[:min(E, GRID * BLOCK)] == 0)                        # an event whose every term is 0
    # the step end over all signals; then a second step at the next proposal
    before = fit.pars.get()
    fit.finish(sums)
    assert fit.counter.get()[0] == 1
    moved = fit.pars.get()
    assert not np.array_equal(moved, before)
    cleared = fit.norms.get()
    assert np.all(cleared[fit.hist_cols] == 0)                                 # members' slots cleared
    assert np.array_equal(cleared[fit.dense_cols], norms[fit.dense_cols])      # dense columns' slots survive
    sums2, _, norms2 = fit.in_place_sums(evaluate_kernels=True)                # (zero launch skipped: cleared by the finish)
    got2 = sums2.get().view(np.uint64)
    want2, _, norms_w2 = fit.materialised_sums()
    print("step 2: %d differ; norms %s" % (int(np.sum(got2 != want2)), list(norms2)))
    assert np.array_equal(got2, want2)
    assert np.array_equal(norms2, norms_w2)
    if E > 1 and np.any(norms > 0):
        assert not np.array_equal(got2, got)                                   # (the second step is another sum)
    return want


def table_1d(rng, n, centre, width):
    t = centre + width * rng.standard_normal(n)
    return np.stack([t + 0.2 * rng.standard_normal(n), t], axis=1).astype(np.float32)


def events_with_dataset(x, dataset=0.0):
    x = np.asarray(x, np.float32).reshape(len(x), -1)
    return np.concatenate([x, np.full((len(x), 1), dataset, np.float32)], axis=1)


def scale_and_resolution(truth_field):
    return [pdfz.ScaleSystematic(0, [0]), pdfz.ResolutionScaleSystematic(0, truth_field, [1])]


def test_case_a_histogram_and_kernel():
    rng = np.random.default_rng(1)
    tables = [table_1d(rng, 20000, 4.0, 2.0), table_1d(rng, 3000, 6.0, 0.4)]
    events = events_with_dataset(rng.uniform(0.5, 9.5, 877))
    fit = Fit("hk", tables, 2, 1, [0.0], [10.0], [25], scale_and_resolution(1), events, [0.01, -0.02])
    try:
        check(fit)
    finally:
        fit.close()


def test_case_b_seventeen_columns_two_passes():
    rng = np.random.default_rng(2)
    kinds = "k" + "h" * 14 + "kk"            # kernel columns at 0, 15 and 16: the second pass of sixteen holds one
    tables = []
    for j, kind in enumerate(kinds):
        n = 500 if kind == "k" else 2000
        t = rng.uniform(0.5 + 0.4 * j, 3.0 + 0.4 * j, n)
        tables.append(np.stack([t + 0.3 * rng.standard_normal(n), rng.uniform(0, 1, n), t], axis=1).astype(np.float32))
    E = 16384 + 37                           # some lanes take two events, most one
    events = events_with_dataset(np.stack([rng.uniform(0, 10, E), rng.uniform(0, 1, E)], axis=1))
    fit = Fit(kinds, tables, 3, 2, [0.0, 0.0], [10.0, 1.0], [8, 6], scale_and_resolution(2), events, [0.02, 0.03])
    try:
        check(fit)
    finally:
        fit.close()


def test_case_c_two_data_sets_empty_members_and_log_free_events():
    rng = np.random.default_rng(3)
    kinds = "hkhk"
    tables = [table_1d(rng, 5000, 4.0, 2.0), table_1d(rng, 800, 6.0, 0.5), table_1d(rng, 3000, 5.0, 1.0),
              table_1d(rng, 600, 3.0, 0.5)]
    # members 2 and 3 also read parameter 2, a shift that takes every one of their samples out of the domain:
    # norm 0, a NaN column
    common = scale_and_resolution(1)
    leaving = common + [pdfz.ShiftSystematic(0, [2])]
    x = np.concatenate([rng.uniform(0.5, 9.5, 700), [-3.0, 10.0, 25.0, np.nan], rng.uniform(0.5, 9.5, 40)])
    dataset = np.concatenate([np.zeros(704), np.ones(40)])     # the last 40: events of the other data set (0)
    events = np.stack([x, dataset], axis=1).astype(np.float32)
    fit = Fit(kinds, tables, 2, 1, [0.0], [10.0], [25], common, events, [0.01, 0.02, 500.0],
              member_systematics=[common, common, leaving, leaving])
    try:
        # the shift must stay where it is: fixed (width -1), like a fixed parameter of a walk
        width = fit.jump_width.get()
        width[-1] = -1.0
        fit.jump_width.set(width)
        want = check(fit, expect_log_free_lanes=True)
        norms = fit.materialised_sums()[2]
        assert norms[2] == 0 and norms[3] == 0 and norms[0] > 0 and norms[1] > 0
        zero = np.float64(0.0).view(np.uint64)
        assert np.all(want[700:744] == zero)       # outside the domain or of the other data set: no log term
    finally:
        fit.close()


@pytest.mark.parametrize("nevents", [1, 0])
def test_case_d_one_event_and_none(nevents):
    rng = np.random.default_rng(4)
    tables = [table_1d(rng, 4000, 4.0, 2.0), table_1d(rng, 500, 6.0, 0.4)]
    events = np.array([[5.5, 0.0]], np.float32)[:nevents]
    fit = Fit("hk", tables, 2, 1, [0.0], [10.0], [25], scale_and_resolution(1), events, [0.01, -0.02])
    try:
        want = check(fit)
        if nevents == 0:
            assert np.all(want == 0)               # no events: zeros everywhere
        else:
            assert want[0] != 0 and np.all(want[1:] == 0)
    finally:
        fit.close()


def test_case_e_histogram_beyond_lds():
    """40 x 40 x 40 bins: the group counts the event bins only (sparse plan) and the in-place look-ups read those
    counters, through the descriptors the materialising lookup is given."""
    rng = np.random.default_rng(5)
    n = 30000
    t = rng.uniform(1.0, 9.0, n)
    big = np.stack([t + 0.3 * rng.standard_normal(n), rng.uniform(0, 1, n), rng.uniform(0, 1, n), t], axis=1)
    m = 400
    tk = 6.0 + 0.5 * rng.standard_normal(m)
    small = np.stack([tk + 0.2 * rng.standard_normal(m), rng.uniform(0, 1, m), rng.uniform(0, 1, m), tk], axis=1)
    E = 613
    events = events_with_dataset(np.stack([rng.uniform(0, 10, E), rng.uniform(0, 1, E), rng.uniform(0, 1, E)], axis=1))
    fit = Fit("hk", [big.astype(np.float32), small.astype(np.float32)], 4, 3, [0.0] * 3, [10.0, 1.0, 1.0], [40] * 3,
              scale_and_resolution(3), events, [0.01, 0.02])
    try:
        check(fit)
    finally:
        fit.close()


def test_columns_must_name_every_member_once():
    rng = np.random.default_rng(6)
    hists = [pdfz.EvalHist(table_1d(rng, 100, 4.0, 2.0).ravel(), 2, 1, [0.0], [10.0], [5]) for _ in range(2)]
    group = nll.EvalGroup(hists)
    try:
        for bad in ([0, 0, -1], [0, -1], [0, 1, 2], [0, -2, 1], []):
            with pytest.raises(capi.SxmcError):
                group.SetColumns(bad)
        group.SetColumns([1, -1, 0])
        sums = capi.DeviceArray.zeros(GRID * BLOCK, np.float64)
        with pytest.raises(capi.SxmcError):    # block beyond the kernel's bound
            group.EvalColumnsNllAsync(None, None, 0, sums, sums, sums, sums, sums, sums, 64, 512)
    finally:
        group.close()
        for h in hists:
            h.close()
