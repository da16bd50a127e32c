"""The arithmetic of the step end, whatever order its instructions run in: the member loop of the event sum at every
edge of its unrolling, with and without the lookup-table stores; phase B of finish_nll_jump_pick_combo from registers
(every addend fetched before the partial sums are waited for, -0.0 where a parameter has no constraint, the accept
counter read ahead, every lane deciding for itself); and the clearing stores issued without loads in front of them.

None of that may change a bit.  The references are the project's own: the two-launch step end
(SetCooperativeStepEnd(False): eval_nll_kernel + finish_zero_kernel) over the same steps, and the host replay of the
Metropolis step (tests/step_reference.py), which shares no code with the device.  Every comparison is on bit patterns,
except where the replay's own numbers come from another implementation of the same function (the proposal's normal
deviate, the oracle's NLL): there the project's bounds for those apply (tests/test_gpu_step_replay.py).

Small tables throughout (about 3 000 samples per signal, 1 500 events): the step end does not see the table size.

This file pins the SEQUENTIAL step end.  The other forms that call the same device functions -- the look-ahead pass, the
lockstep sets' joint ends, the one-workgroup end, the fused step -- are walked at the same edges, and at their own limits,
in tests/test_gpu_step_end_forms.py (cases: tests/step_end_form_cases.py).
"""
import copy

import numpy as np
import pytest

from sxmc_amd import capi
from sxmc_amd.mcmc import MCMC
from tests.step_reference import StepReference
from tests.test_gpu_nll import NLL_RTOL, oracle_nll_of_workload
from tests.test_gpu_step_end_table import make_workload

pytestmark = pytest.mark.gpu

SEED = 5


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def close(m):
    capi.synchronize()
    if m._graph is not None:
        m._graph.close()
    for p in m.pdfs:
        p.close()
    m.group.close()


def workload(nsig, nclasses, nbins=(20, 20), nevents=1500):
    """tests/test_gpu_step_end_table.py's workload -- events outside the histogram (bin -1: NaN) in every member, signals
    1 and 2 on one source, from three members on a last member of normalisation 0 -- with seven more events of a data set
    no signal belongs to: bin -2 in every member, one class of their own (so `nclasses` stays the number of classes)."""
    if nclasses == 1:
        return make_workload(nsig, 1, nbins, nevents=nevents)
    w = make_workload(nsig, nclasses - 1, nbins, nevents=nevents - 7)
    other = np.repeat(w.events[:1], 7, axis=0)
    other[:, -1] = 1.0
    w.events = np.ascontiguousarray(np.concatenate([w.events[:700], other, w.events[700:]]))
    return w


def new_chain(w, coop, lut_output, sync_interval, jump_width=None):
    m = MCMC(w, seed=SEED, lut_output=lut_output, consume=True, stream=capi.new_stream())
    m.group.SetCooperativeStepEnd(coop)
    m.group.SetFusedStep(False)
    m.setup(w.events, sync_interval=sync_interval, jump_width=jump_width)
    return m


def record(m):
    """Everything a flush shows of the chain, as bit patterns: the jump buffer's rows, the accept count, both NLLs, both
    vectors, the generators."""
    rows, nacc = m.flush()
    return dict(rows=bits(rows).copy(), nacc=nacc, count=rows.shape[0],
                current_nll=bits(m.current_nll.get()).copy(), proposed_nll=bits(m.proposed_nll.get()).copy(),
                current_vector=bits(m.current_vector.get()).copy(),
                proposed_vector=bits(m.proposed_vector.get()).copy(), rngs=m.rngs.get().copy())


def same(got, want):
    assert got["nacc"] == want["nacc"] and got["count"] == want["count"], (got["nacc"], want["nacc"], got["count"])
    for k in ("rows", "current_nll", "proposed_nll", "current_vector", "proposed_vector", "rngs"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4])


def run(w, coop, graph_steps, nsteps, flush_every, lut_output=False, jump_width=None):
    """nsteps steps, flushed every flush_every; launched one by one, or replayed from a graph of graph_steps recorded
    steps wherever they fit.  Returns the flushes' records, the lookup table's bits and the launches per step."""
    m = new_chain(w, coop, lut_output, flush_every, jump_width)
    try:
        out, launches = [], set()
        for first in range(0, nsteps, flush_every):
            n = min(flush_every, nsteps - first)
            if first == 0:
                m.step()                                        # (one step launched directly before any is recorded)
                n -= 1
            m.steps(n, graph_steps)
            out.append(record(m))                               # (flush(): raises if a workgroup gave up waiting)
            launches.add(m.group.LastStepLaunches())
            assert m.group.StepEndTimeouts() == 0
        lut = bits(m.lut.get()).copy() if lut_output else None
    finally:
        close(m)
    return out, lut, launches


# ------------------------------------------------------------------------ members and rows at every edge of the unrolling
# 20 x 20 bins: 300 classes are two full virtual blocks of 128 rows and a partial one; 127 / 128 / 129 sit on each side of
# one block.  Where rows x members <= 256 the step end would be the one-workgroup form, which small problems take instead:
# the one-class cases get histograms of more than 65 536 words in all, which that form is not offered for.  (One member
# with one class or a block's worth of them is that form's whatever the histogram; one member is walked at 300 classes.)
# The last figure: launches per step with the cooperative step end -- the fill + ONE step-end launch, 2; 3 where the
# fill itself takes two launches (12 histograms of 64 x 90 bins do not fit one launch's LDS).  The two-launch form: one more.
CASES = [(1, 300, (20, 20), 2), (12, 300, (20, 20), 2), (16, 300, (20, 20), 2), (17, 300, (20, 20), 2),
         (12, 127, (20, 20), 2), (12, 128, (20, 20), 2), (12, 129, (20, 20), 2), (12, 1, (64, 90), 3),
         (17, 129, (20, 20), 2), (16, 129, (20, 20), 2), (16, 1, (64, 65), 2), (17, 1, (64, 65), 2)]


@pytest.mark.parametrize("nsig,nclasses,nbins,per_step", CASES)
def test_class_rows_walk_the_two_launch_chain(nsig, nclasses, nbins, per_step):
    """The class form: rows are event classes, nothing is stored.  64 steps, flushed twice."""
    w = workload(nsig, nclasses, nbins)
    want, _, want_launches = run(w, False, 0, 64, 32)
    assert want_launches == {per_step + 1}, want_launches      # the event sum and the step end as two launches
    if nsig >= 3:
        m = new_chain(w, True, False, 8)
        assert m.normalizations.get()[-1] == 0                  # (the member whose samples all lie outside)
        close(m)
    assert 0 < sum(r["nacc"] for r in want) < 64
    for graph_steps in (0, 8):
        got, _, launches = run(w, True, graph_steps, 64, 32)
        assert launches == {per_step}, launches
        for g, r in zip(got, want):
            same(g, r)


@pytest.mark.parametrize("nsig,nclasses,nevents", [(12, 300, 1500), (16, 40, 129), (17, 300, 1500)])
def test_event_rows_store_the_lookup_table(nsig, nclasses, nevents):
    """lut_output=True: rows are the events themselves and every member stores its lookup-table row.  The chain and the
    table, bit for bit, against the two-launch form."""
    w = workload(nsig, nclasses, (20, 20), nevents=nevents)
    want, want_lut, want_launches = run(w, False, 0, 48, 24, lut_output=True)
    lut = want_lut.view(np.float32).reshape(nsig, nevents)
    other = w.events[:, -1] == 1.0
    assert np.count_nonzero(other) == 7
    # every member: 0 for the events of the other data set (bin -2); NaN outside the histogram (bin -1) -- and, in the
    # member of normalisation 0, wherever 0 / 0 is stored as it is (and counted as 0)
    assert np.all(lut[:, other] == 0)
    assert np.all(np.isnan(lut[-1][~other])) and np.any(np.isnan(lut[0])) and np.any(lut[0] > 0)
    for graph_steps in (0, 8):
        got, got_lut, launches = run(w, True, graph_steps, 48, 24, lut_output=True)
        assert launches == {2} and want_launches == {3}, (launches, want_launches)
        for g, r in zip(got, want):
            same(g, r)
        assert np.array_equal(got_lut, want_lut), np.argwhere(got_lut != want_lut)[:4]


# ------------------------------------------------------------------------ both outcomes of phase B, and its early-outs
def wide_first_rate(w):
    """The walk's own widths, but the first source's rate jumps by about 3 -- the data put it near 2, to a tenth or two --
    so that a good part of the proposals has a negative rate and few of the others are accepted.  The rates are the
    parameters with sigma = 0 (no constraint term); the systematic's has one."""
    jw = MCMC.initial_jump_widths(_Widths(w))
    jw[0] = np.float32(3.0)
    return jw


class _Widths:
    def __init__(self, w):
        self.w, self.nparameters, self.nsignals = w, w.nparameters, w.nsignals


NSTEPS, FLUSH = 80, 20
_followed = {}


class Replay:
    """One chain beside the host replay of its steps (tests/step_reference.py), one decided step at a time: the device's
    proposal within the project's bound on a device normal (tests/test_gpu_step_replay.py, follow()), its NLL against the
    oracle's within NLL_RTOL, and from those the replay's decision, counters, jump-buffer rows, current values and
    generator offsets, bit for bit.  Shared by followed() below and tests/test_gpu_step_end_forms.py.
    m: a chain after setup(), `rows` its jump buffer's rows; events: the chain's own, where they are not w's."""

    def __init__(self, m, w, seed, rows, events=None):
        capi.synchronize()                                      # (the set-up's first proposal is drawn on the chain's stream)
        self.m, self.rows = m, rows
        self.w = w
        if events is not None:
            self.w = copy.copy(w)
            self.w.events = events
        jw = m.jump_width.get()
        self.ref = StepReference(seed, jw, m.current_vector.get(), m.current_nll.get()[0], rows)
        self.ref.first_proposal()
        self.free = jw > 0
        self.width = np.clip(jw.astype(np.float64), 0.0, None)
        self.v_cur, self.nll_cur = m.current_vector.get(), m.current_nll.get()[0]
        self.k = self.accepted = self.negative = 0

    def proposal(self, vp):
        """vp is what the replay proposes now: the project's bound on a device normal."""
        ref = self.ref
        tol = 8e-12 * self.width + 2.0 ** -52 * np.abs(ref.v_proposed)
        assert np.all(np.abs(vp - ref.v_proposed) <= tol), (self.k, vp, ref.v_proposed)
        assert np.array_equal(bits(vp[~self.free]), bits(self.v_cur[~self.free]))

    def before(self):
        """Ahead of a step's launch: the pending proposal and the counters."""
        m = self.m
        self.vp = m.proposed_vector.get()
        self.proposal(self.vp)
        self.acc_before, self.count = int(m.accept_counter.get()[0]), int(m.jump_counter.get()[0])
        assert (self.acc_before, self.count) == (self.ref.accepted, self.ref.count)

    def oracle(self, v):
        return oracle_nll_of_workload(self.w, v)[0]

    def refused_unseen(self):
        """A step the device decided and then overwrote the NLL of (the look-ahead pass's A-step after a rejection): the
        replay decides it from the oracle's NLL, and it must be a rejection too."""
        rec = self.ref.step(self.oracle(self.vp), v_proposed=self.vp)
        assert not rec["accept"], (self.k, rec)
        self.k += 1
        self.count += 1

    def after(self, vp, check_nll):
        """The step over proposal vp has run: its NLL, the decision and everything the decision implies."""
        m, ref, k = self.m, self.ref, self.k
        P = vp.size
        got = m.proposed_nll.get()[0]
        if np.any(vp[:self.w.nsources] < 0):                    # nll_kernels.cpp:176-179: 1e18, and a finite chain says no
            self.negative += 1
            assert got == 1e18, (k, got)
        elif check_nll:
            want = self.oracle(vp)
            assert got == want or abs(got - want) <= NLL_RTOL * abs(want), (k, got, want)
        rec = ref.step(got, v_proposed=vp)
        accepted = int(m.accept_counter.get()[0]) - self.acc_before
        assert accepted == int(rec["accept"]), (k, rec)
        assert not (got == 1e18 and accepted), k
        self.v_cur = vp if accepted else self.v_cur
        self.nll_cur = got if accepted else self.nll_cur
        assert np.array_equal(bits(m.current_vector.get()), bits(self.v_cur)), k
        assert bits(m.current_nll.get())[0] == bits(np.array([self.nll_cur]))[0], k
        assert int(m.jump_counter.get()[0]) == ref.count == self.count + 1
        jb = m.jump_buffer.get().reshape(self.rows, P + 1)
        assert np.array_equal(bits(jb[:ref.count]), bits(ref.jump_buffer[:ref.count])), (k, self.count)
        assert np.array_equal(bits(jb[self.count, :P]), bits(self.v_cur.astype(np.float32)))
        assert bits(jb[self.count, P:])[0] == bits(np.array([self.nll_cur], np.float64).astype(np.float32))[0]
        st = m.rngs.get().reshape(P, 4)
        assert [int(o) for o in st[:, 2]] == ref.offsets, k
        self.k += 1
        self.accepted += accepted

    def flushed(self):
        """The chain's flush() has reset its counters."""
        self.ref.accepted = self.ref.count = 0


def followed(nsig):
    """The cooperative step end launched one by one, every step followed by the host replay.  Returns the flushes'
    records (computed once, shared, never modified)."""
    if nsig in _followed:
        return _followed[nsig]
    w = workload(nsig, 300)
    jw = wide_first_rate(w)
    sigmas = w.parameter_sigmas()
    assert np.count_nonzero(sigmas == 0) == w.nsources and np.count_nonzero(sigmas > 0) >= 1
    m = new_chain(w, True, False, FLUSH, jw)
    r = Replay(m, w, SEED, FLUSH)
    out, accepted_total = [], 0
    for k in range(NSTEPS):
        r.before()
        m.step()
        capi.synchronize()
        # (the fill + ONE step-end launch; a chain's first step zeroes the histograms in a launch of its own before them)
        assert m.group.LastStepLaunches() == (3 if k == 0 else 2), (k, m.group.LastStepLaunches())
        assert m.group.StepEndTimeouts() == 0
        r.after(r.vp, k % 8 == 0)
        if (k + 1) % FLUSH == 0:
            rec = record(m)
            assert (rec["nacc"], rec["count"]) == (r.ref.accepted, r.ref.count)
            accepted_total += rec["nacc"]
            out.append(rec)
            r.flushed()
    close(m)
    assert r.negative >= 1, r.negative
    assert 0 < accepted_total < NSTEPS, accepted_total
    _followed[nsig] = out
    return out


@pytest.mark.parametrize("nsig", [12, 17])
def test_phase_b_follows_the_host_replay(nsig):
    """80 steps that go both ways, with proposals of a negative source rate among them, step by step beside the host
    replay: the decision, the counters, the jump buffer's row, both current values and the generators after every step."""
    followed(nsig)


@pytest.mark.parametrize("coop,graph_steps", [(False, 0), (True, 0), (True, 8)])
@pytest.mark.parametrize("nsig", [12, 17])
def test_phase_b_is_the_same_in_every_form(nsig, coop, graph_steps):
    """The same 80 steps through the two-launch step end, and through the cooperative one without a read-back between
    the steps of a flush, launched one by one and replayed from a graph: the followed chain's records after every flush."""
    want = followed(nsig)
    w = workload(nsig, 300)
    got, _, launches = run(w, coop, graph_steps, NSTEPS, FLUSH, jump_width=wide_first_rate(w))
    assert launches == ({2} if coop else {3})
    assert len(got) == len(want) == NSTEPS // FLUSH
    for g, r in zip(got, want):
        same(g, r)


# ------------------------------------------------------------------------ vectors longer than the finisher stages
def many_sources(nsig):
    """nsig small signals, each its own source (no systematic): nsig parameters and nsig signals -- beyond 256 the step
    end totals the NLL sequentially, from the normalisations, BEHIND its wait for the partial sums, so nothing may have
    cleared them by then.  Signal j sits at 2 + 6 j / nsig in the first observable: every normalisation is far from 0."""
    from sxmc_amd import workloads
    from tests.test_gpu_step_end_table import HI, LO, make_events
    rng = np.random.default_rng(11)
    signals = []
    for j in range(nsig):
        n = 400 + j
        e = rng.normal(2.0 + 6.0 * j / nsig, 1.0, size=n)
        r = 6.0 * rng.uniform(0.0, 1.0, size=n) ** (1.0 / 3.0)
        tab = np.stack([e, r, np.zeros(n)], axis=1).astype(np.float32)
        signals.append(workloads.Signal(tab, 3, nexpected=5.0 + 0.01 * j, source_id=j))
    ev = make_events(rng, (20, 20), 300, 1500)
    return workloads.Workload("long vectors", 2, LO, HI, [20, 20], signals, [], [], ev, "S = P = %d" % nsig)


@pytest.mark.parametrize("nsig", [256, 257])
def test_long_vectors_walk_the_two_launch_chain(nsig):
    """256 parameters and signals are staged, 257 are not: both through the cooperative step end, launched one by one and
    replayed, against the two-launch form -- and the first proposal's NLL against the oracle."""
    w = many_sources(nsig)
    assert w.nparameters == nsig and w.nsignals == nsig
    # (every rate jumps by 0.04: the walk's own widths, shared among so many parameters, move the NLL by a hundredth)
    jw = np.full(nsig, 0.04, np.float32)
    m = new_chain(w, True, False, 8, jw)
    try:
        capi.synchronize()                                      # (the set-up's first proposal is drawn on the chain's stream)
        assert np.count_nonzero(m.normalizations.get() > 100) == nsig
        vp = m.proposed_vector.get()
        m.step()
        capi.synchronize()
        got, want = m.proposed_nll.get()[0], oracle_nll_of_workload(w, vp)[0]
        assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
        assert m.group.StepEndTimeouts() == 0
        # every parameter is free: every one has a new proposal, a normal deviate's 0.04 away from the current value
        away = np.abs(m.proposed_vector.get() - m.current_vector.get())
        assert np.all(away > 0) and np.all(away < 0.04 * 6.7), np.flatnonzero(~(away > 0))
    finally:
        close(m)
    want, _, want_launches = run(w, False, 0, 32, 16, jump_width=jw)
    assert want_launches == {3}, want_launches
    assert 0 < sum(r["nacc"] for r in want) < 32
    for graph_steps in (0, 8):
        got, _, launches = run(w, True, graph_steps, 32, 16, jump_width=jw)
        assert launches == {2}, launches
        for g, r in zip(got, want):
            same(g, r)
