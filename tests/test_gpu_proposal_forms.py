"""The correlated proposal through every form sxmc_group_step_async ends a step in -- one-workgroup, cooperative,
two-launch, fused -- on the shapes of tests/step_end_form_cases.py: with a factor set on the group
(sxmc_group_set_proposal_factor) the forms walk each other's chain as bytes, and that chain is the host replay's
(tests/step_reference_cov.py).  The look-ahead pass and lockstep sets refuse such a group.

The walks, their records and their comparison are those of tests/test_gpu_step_end_forms.py (64 steps flushed twice,
eager and replayed from a graph of 8 steps, WHICH FORM RAN asserted from the launches per step); the reference is again
the two-launch sequential chain, here with the same factor set.  The factor is the re-tuning's own
(sxmc_proposal_factor) from correlated rows with the chain's widths, so the proposals stay of the walk's size and both
outcomes of a step occur."""
import numpy as np
import pytest

from sxmc_amd import capi, nll
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import LockstepChains, LookaheadWalk, MCMC
from tests import step_end_form_cases as cases
from tests import step_reference_cov as cov
from tests.test_gpu_step_end_arith import Replay, bits, close, same
from tests.test_gpu_step_end_forms import (FLUSH, GRAPH, IN_THE_FILL, NSTEPS, ONE_LAUNCH, SEED, TWO_LAUNCHES, fills,
                                           new_chain, walk, widths_of)

pytestmark = pytest.mark.gpu


def factor_for(jw):
    """(L as [P, P], its device image): the re-tuning's factor for strongly correlated rows and widths jw."""
    P = jw.size
    rng = np.random.default_rng(77 + P)
    rows = (rng.standard_normal((200, P)) + 1.5 * rng.standard_normal((200, 1))) * (1.0 + np.arange(P) % 3)
    rows = np.concatenate([rows, np.zeros((200, 1))], axis=1).astype(np.float32)
    image, used = nll.proposal_factor(rows, jw, 0.05)
    assert used == 0.05
    L = image.reshape(P, P).T.copy()
    assert np.count_nonzero(np.tril(L, -1)) > 0 or np.count_nonzero(jw > 0) < 2
    return L, image


def chain_with_factor(w, jw, **kw):
    m = new_chain(w, jump_width=jw, **kw)
    L, image = factor_for(m.jump_width.get())
    m._factor_image = DeviceArray(image)                       # (borrowed by the group: lives as long as the chain)
    m.group.SetProposalFactor(m._factor_image)
    return m, L


_reference = {}


def reference(case, w, jw, **kw):
    key = (repr(case), tuple(sorted(kw.items())))
    if key not in _reference:
        m, _ = chain_with_factor(w, jw, coop=False, fused=False, tail=False, **kw)
        try:
            out, _, ends = walk(m, 0)
        finally:
            close(m)
        assert ends == {TWO_LAUNCHES}, ends
        assert 0 < sum(r["nacc"] for r in out) < NSTEPS, [r["nacc"] for r in out]
        _reference[key] = out
    return _reference[key]


def check_form(case, end, ordering=False, graphs=(0, GRAPH), fixed=None, **switches):
    w = case.workload()
    jw = widths_of(case, w, fixed)
    kw = dict(ordering=True) if ordering else {}
    want = reference(case if fixed is None else (case, tuple(fixed)), w, jw, **kw)
    for graph_steps in graphs:
        m, _ = chain_with_factor(w, jw, **switches, **kw)
        try:
            got, _, ends = walk(m, graph_steps)
        finally:
            close(m)
        assert ends == {end}, (case, graph_steps, ends)
        assert len(got) == len(want)
        for g, r in zip(got, want):
            same(g, r)


# 16 / 17 members on each side of the member loop's sixteen; 127 / 128 / 129 rows on each side of a block of 128
COOPERATIVE = [cases.Case(16, 300), cases.Case(17, 300), cases.Case(12, 127), cases.Case(12, 128), cases.Case(12, 129)]


@pytest.mark.parametrize("case", COOPERATIVE, ids=repr)
def test_cooperative_end_walks_the_two_launch_chain(case):
    """(None of these shapes is small enough for the one-workgroup end: ONE launch is the cooperative end.)"""
    assert not case.one_workgroup
    check_form(case, ONE_LAUNCH, coop=True)


@pytest.mark.parametrize("case", cases.TAIL_TAKEN[:3], ids=repr)
def test_one_workgroup_end_walks_the_two_launch_chain(case):
    """16 x 16, 17 x 15 and 1 x 256 look-ups (the cooperative end switched off: ONE launch is then this form)."""
    assert case.one_workgroup
    check_form(case, ONE_LAUNCH, coop=False, tail=True)


@pytest.mark.parametrize("case", cases.FUSED, ids=repr)
def test_fused_step_walks_the_two_launch_chain(case):
    check_form(case, IN_THE_FILL, ordering=True, coop=True, fused=True)


@pytest.mark.parametrize("form", ["cooperative", "one workgroup"])
def test_fixed_parameters_between_free_ones(form):
    """Rates 1 and 3 and the systematic fixed, free parameters behind them: a fixed parameter's z is 0 in the product of
    every free parameter after it, whatever the LDS held (the factor here has zero columns for them, so anything finite
    would pass unnoticed -- but not what a fill kernel may have left there; the step-end test has the non-zero columns)."""
    case = cases.Case(12, 300) if form == "cooperative" else cases.TAIL_TAKEN[0]
    w = case.workload()
    fixed = [i in (1, 3, w.nparameters - 1) for i in range(w.nparameters)]
    if form == "cooperative":
        check_form(case, ONE_LAUNCH, fixed=fixed, coop=True)
    else:
        check_form(case, ONE_LAUNCH, fixed=fixed, coop=False, tail=True)


def test_the_factor_changes_the_chain_and_null_restores_it():
    """The diagonal chain, the correlated one, and the diagonal one again after SetProposalFactor(None): the first and
    the last are the same bytes, the middle one is not."""
    case = cases.Case(12, 129)
    w = case.workload()
    jw = widths_of(case, w)
    records = []
    for with_factor in (False, True, False):
        m, _ = chain_with_factor(w, jw, coop=True)
        try:
            if not with_factor:
                m.group.SetProposalFactor(None)
            records.append(walk(m, 0)[0])
        finally:
            close(m)
    for a, b in zip(records[0], records[2]):
        same(a, b)
    assert not np.array_equal(records[0][0]["rows"], records[1][0]["rows"])


class ReplayCov(Replay):
    """tests/test_gpu_step_end_arith.py's Replay with the correlated law.  The bound on a pending proposal: the device's
    deviates are within 8e-12 of the replay's (the project's bound on a device normal), so d_i within
    8e-12 sum_j |L_ij|; its i + 1 fused multiply-adds and the final addition round once each, at most (i + 2) 2^-52 of the
    largest magnitude on the way, sum_j |L_ij z_j| + |v_i|."""

    def __init__(self, m, w, seed, rows, L):
        super().__init__(m, w, seed, rows)
        jw = m.jump_width.get()
        self.ref = cov.StepReferenceCov(seed, jw, m.current_vector.get(), m.current_nll.get()[0], rows, factor=L)
        self.ref.first_proposal()
        self.L = np.abs(L)
        self.first = True

    def proposal(self, vp):
        ref = self.ref
        if self.first:                       # (the set-up's proposal: pick_new_vector's, the diagonal law)
            tol = 8e-12 * self.width + 2.0 ** -52 * np.abs(ref.v_proposed)
        else:
            n = np.arange(vp.size) + 2
            tol = 8e-12 * self.L.sum(axis=1) + n * 2.0 ** -52 * (self.L @ np.abs(ref.last_z) + np.abs(ref.v_proposed))
        assert np.all(np.abs(vp - ref.v_proposed) <= tol), (self.k, vp, ref.v_proposed)
        assert np.array_equal(bits(vp[~self.free]), bits(self.v_cur[~self.free]))
        self.first = False


def test_two_launch_end_follows_the_host_replay():
    """The reference of the tests above, step by step beside the replay: its proposals within the bound of ReplayCov,
    its NLL against the oracle's, and from those the replay's decisions, rows, counters and offsets bit for bit."""
    case = cases.Case(12, 129)
    w = case.workload()
    m, L = chain_with_factor(w, widths_of(case, w), coop=False, tail=False, rows=NSTEPS)
    try:
        r = ReplayCov(m, w, SEED, NSTEPS, L)
        for k in range(NSTEPS):
            r.before()
            m.step()
            capi.synchronize()
            assert m.group.LastStepLaunches() - fills(m) == TWO_LAUNCHES + (k == 0), k
            r.after(r.vp, k % 8 == 0)
        assert 0 < r.accepted < NSTEPS, r.accepted
        # the proposals were correlated: not the diagonal law's
        diag = m.current_vector.get() + np.clip(m.jump_width.get(), 0, None).astype(np.float64) * r.ref.last_z
        assert np.max(np.abs(m.proposed_vector.get() - diag)) > 1e-6
    finally:
        close(m)


def test_256_parameters_take_the_factor_and_257_are_refused():
    """The one-workgroup end over 256 members and parameters, staged at exactly kStage; one more is SXMC_ERR_SHAPE at the
    step, before anything is launched."""
    case = cases.TAIL_TAKEN[3]
    assert case.members == 256
    check_form(case, ONE_LAUNCH, graphs=(0,), coop=False, tail=True)   # (eager only: hundreds of evaluators per chain)
    case = cases.TAIL_NOT_TAKEN[2]
    w = case.workload()
    assert w.nparameters == 257
    m = new_chain(w, jump_width=widths_of(case, w))
    try:
        m._factor_image = DeviceArray.zeros(257 * 257, np.float64)
        m.group.SetProposalFactor(m._factor_image)
        with pytest.raises(capi.SxmcError) as e:
            m.step()
        assert e.value.code == capi.ERR_SHAPE and "256 parameters" in e.value.msg
        m.group.SetProposalFactor(None)
        m.step()
        capi.synchronize()
        assert int(m.jump_counter.get()[0]) == 1
    finally:
        close(m)


def test_multigroup_entry_points_refuse_a_factor():
    """sxmc_multigroup_step_async and sxmc_multigroup_lookahead_step_async: SXMC_ERR_STATE with the reason;
    sxmc_group_lookahead_supported: 0, and the group's fill form is left as it was."""
    case = cases.LOOKAHEAD[2]
    w = case.workload()
    m, _ = chain_with_factor(w, widths_of(case, w))
    la = None
    try:
        form_before = m.group.FillForm()
        assert not m.group.LookaheadSupported()
        assert m.group.FillForm() == form_before
        la = LookaheadWalk(m, threads=0)
        la.bind(w.events)
        with pytest.raises(capi.SxmcError) as e:
            la.one_pass()
        assert e.value.code == capi.ERR_STATE and "proposal factor" in e.value.msg and "look-ahead" in e.value.msg
        m.group.SetProposalFactor(None)
        assert m.group.LookaheadSupported()
    finally:
        if la is not None:
            la.close()
        close(m)
    w = cases.lockstep_workload(16)
    stream = capi.new_stream()
    base = MCMC(w, seed=1, lut_output=False, consume=True, stream=stream)
    chains, ls = [], None
    try:
        for c in range(2):
            chains.append(new_chain(w, seed=SEED + c, stream=stream, share_with=base,
                                    data=cases.lockstep_events(16, cases.LOCKSTEP_CLASSES[c], c)))
        L, image = factor_for(chains[1].jump_width.get())
        chains[1]._factor_image = DeviceArray(image)
        chains[1].group.SetProposalFactor(chains[1]._factor_image)
        ls = LockstepChains(chains)
        with pytest.raises(capi.SxmcError) as e:
            ls.step()
        assert e.value.code == capi.ERR_STATE and "proposal factor" in e.value.msg and "lockstep" in e.value.msg
        chains[1].group.SetProposalFactor(None)
        ls.step()
        capi.synchronize()
    finally:
        if ls is not None:
            ls.close()
        for m in chains[::-1]:
            close(m)
        close(base)
