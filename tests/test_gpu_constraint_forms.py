"""Correlated constraints through every form sxmc_group_step_async ends a step in -- one-workgroup, cooperative,
two-launch, fused -- on shapes of tests/step_end_form_cases.py whose rates carry constraints too: with a whitening matrix
set on the group (sxmc_group_set_constraint_whitening) the forms walk each other's chain as bytes, that chain is the host
replay's (tests/step_reference_constraints.py), and W = I walks the chain of no matrix at all, as bytes, in every form.
The look-ahead pass and lockstep sets refuse such a group.  (The columns step end of the mixed walk:
tests/test_gpu_constraint_cpp.py.)

The walks, their records and their comparison are those of tests/test_gpu_step_end_forms.py (64 steps flushed twice,
eager and replayed from a graph of 8 steps, WHICH FORM RAN asserted from the launches per step); the reference is again
the two-launch sequential chain, here with the same matrix set."""
import numpy as np
import pytest

from sxmc_amd import capi, workloads
from sxmc_amd.mcmc import LockstepChains, LookaheadWalk, MCMC
from tests import step_end_form_cases as cases
from tests import step_reference_constraints as sc
from tests.test_gpu_step_end_arith import Replay, close, same
from tests.test_gpu_step_end_forms import (GRAPH, IN_THE_FILL, NSTEPS, ONE_LAUNCH, SEED, TWO_LAUNCHES, FLUSH, fills,
                                           walk, widths_of)

pytestmark = pytest.mark.gpu

LAWS = ("none", "identity", "correlated")


class Constrained(workloads.Workload):
    """A workload of step_end_form_cases.py whose rates carry constraints too (0.3, but for rate 0, which keeps none), so
    that the correlations reach across rates and the systematic."""

    def __init__(self, w):
        self.__dict__.update(w.__dict__)
        sig = np.asarray(w.parameter_sigmas(), np.float64).copy()
        sig[:w.nsources] = 0.3
        if w.nsources > 2:
            sig[0] = 0.0
        self._sigmas = sig

    def parameter_sigmas(self):
        return self._sigmas.copy()


_workloads = {}


def constrained(case):
    if repr(case) not in _workloads:
        _workloads[repr(case)] = Constrained(case.workload())
    return _workloads[repr(case)]


def rho_of(w, law):
    if law == "none":
        return None
    P = w.nparameters
    if law == "identity":
        return np.eye(P)
    idx = np.flatnonzero(w.parameter_sigmas() > 0)
    assert idx.size >= 2
    return sc.block_matrix(P, [(idx, sc.random_correlation(idx.size, np.random.default_rng(40 + P), 0.8))])


def new_chain(w, law, jw, coop=None, fused=False, tail=True, ordering=False, rows=FLUSH):
    m = MCMC(w, seed=SEED, lut_output=False, consume=True, stream=capi.new_stream())
    if coop is not None:
        m.group.SetCooperativeStepEnd(coop)
    m.group.SetFusedStep(fused)
    m.group.SetTailKernel(tail)
    if ordering:
        m.group.SetOrdering(True, force=True)
    m.set_constraint_correlation(rho_of(w, law))
    m.setup(w.events, sync_interval=rows, jump_width=jw)
    return m


_reference = {}


def reference(case, law, ordering=False):
    """The two-launch sequential chain under `law`: walked once, shared, never modified."""
    key = (repr(case), law, ordering)
    if key not in _reference:
        w = constrained(case)
        m = new_chain(w, law, widths_of(case, w), coop=False, fused=False, tail=False, ordering=ordering)
        try:
            out, _, ends = walk(m, 0)
        finally:
            close(m)
        assert ends == {TWO_LAUNCHES}, ends
        assert 0 < sum(r["nacc"] for r in out) < NSTEPS, [r["nacc"] for r in out]
        _reference[key] = out
    return _reference[key]


def check_form(case, end, ordering=False, graphs=(0, GRAPH), **switches):
    w = constrained(case)
    jw = widths_of(case, w)
    want = {law: reference(case, law, ordering) for law in LAWS}
    # W = I is the chain of no matrix, as bytes; the correlated chain is another one
    for a, b in zip(want["identity"], want["none"]):
        same(a, b)
    assert not np.array_equal(want["correlated"][-1]["rows"], want["none"][-1]["rows"])
    for law in LAWS:
        for graph_steps in graphs:
            m = new_chain(w, law, jw, ordering=ordering, **switches)
            try:
                got, _, ends = walk(m, graph_steps)
            finally:
                close(m)
            assert ends == {end}, (case, law, graph_steps, ends)
            assert len(got) == len(want[law])
            for g, r in zip(got, want[law]):
                same(g, r)


@pytest.mark.parametrize("case", [cases.Case(17, 300), cases.Case(12, 129)], ids=repr)
def test_cooperative_end_walks_the_two_launch_chain(case):
    assert not case.one_workgroup
    check_form(case, ONE_LAUNCH, coop=True)


@pytest.mark.parametrize("case", cases.TAIL_TAKEN[:2], ids=repr)
def test_one_workgroup_end_walks_the_two_launch_chain(case):
    assert case.one_workgroup
    check_form(case, ONE_LAUNCH, coop=False, tail=True)


@pytest.mark.parametrize("case", cases.FUSED, ids=repr)
def test_fused_step_walks_the_two_launch_chain(case):
    check_form(case, IN_THE_FILL, ordering=True, coop=True, fused=True)


def test_null_restores_the_uncorrelated_chain():
    case = cases.Case(12, 129)
    w = constrained(case)
    m = new_chain(w, "correlated", widths_of(case, w), coop=True)
    try:
        assert m.ConstraintWhitening().shape == (w.nparameters, w.nparameters)
        m.set_constraint_correlation(None)
        assert m.ConstraintWhitening() is None
        m.setup(w.events, sync_interval=FLUSH, jump_width=widths_of(case, w))
        got, _, _ = walk(m, 0)
    finally:
        close(m)
    # (the generators went on from the first set-up's draw: compare with a chain that drew it twice as well)
    m = new_chain(w, "none", widths_of(case, w), coop=True)
    try:
        m.setup(w.events, sync_interval=FLUSH, jump_width=widths_of(case, w))
        want, _, _ = walk(m, 0)
    finally:
        close(m)
    for g, r in zip(got, want):
        same(g, r)


class ReplayConstrained(Replay):
    """tests/test_gpu_step_end_arith.py's Replay with the constraints' law: the oracle's NLL (independent constraints)
    with its constraint terms exchanged for the whitened ones.  The exchange is three sums of a few terms of order one
    beside an NLL in the thousands: far inside NLL_RTOL."""

    def __init__(self, m, w, seed, rows, W):
        super().__init__(m, w, seed, rows)
        self.W = W
        self.means, self.sigmas = w.parameter_means().astype(np.float64), w.parameter_sigmas().astype(np.float64)

    def oracle(self, v):
        plain = super().oracle(v)
        if plain == 1e18:
            return plain
        out = plain - float(np.sum(sc.penalties(v, self.means, self.sigmas))) \
            + float(np.sum(sc.penalties(v, self.means, self.sigmas, self.W)))
        return out


def test_two_launch_end_follows_the_host_replay():
    """The reference of the tests above, step by step beside the replay: its NLL against the oracle's with the whitened
    constraint terms, and from that the replay's decisions, rows, counters and offsets bit for bit."""
    case = cases.Case(12, 129)
    w = constrained(case)
    m = new_chain(w, "correlated", widths_of(case, w), coop=False, tail=False, rows=NSTEPS)
    try:
        W = m.ConstraintWhitening()
        assert np.count_nonzero(np.tril(W, -1)) > 0
        r = ReplayConstrained(m, w, SEED, NSTEPS, W)
        differs = 0
        for k in range(NSTEPS):
            r.before()
            m.step()
            capi.synchronize()
            assert m.group.LastStepLaunches() - fills(m) == TWO_LAUNCHES + (k == 0), k
            got = m.proposed_nll.get()[0]
            plain = Replay.oracle(r, r.vp)
            differs += int(got != 1e18 and abs(got - plain) > 1e-9 * abs(plain))
            r.after(r.vp, True)
        assert 0 < r.accepted < NSTEPS, r.accepted
        assert differs > NSTEPS // 2, differs        # (the constraints were the correlated ones, not the independent)
    finally:
        close(m)


def test_multigroup_entry_points_refuse_a_whitening_matrix():
    """sxmc_multigroup_step_async and sxmc_multigroup_lookahead_step_async: SXMC_ERR_STATE with the reason;
    sxmc_group_lookahead_supported: 0, and the group's fill form is left as it was."""
    case = cases.LOOKAHEAD[2]
    w = constrained(case)
    m = new_chain(w, "correlated", widths_of(case, w))
    la = None
    try:
        form_before, info_before = m.group.FillForm(), m.group.LaunchInfo()
        assert not m.group.LookaheadSupported()
        assert m.group.FillForm() == form_before and m.group.LaunchInfo() == info_before
        la = LookaheadWalk(m, threads=0)
        la.bind(w.events)
        with pytest.raises(capi.SxmcError) as e:
            la.one_pass()
        assert e.value.code == capi.ERR_STATE and "constraint whitening" in e.value.msg and "look-ahead" in e.value.msg
        m.group.SetConstraintWhitening(None)
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
            m = MCMC(w, seed=SEED + c, lut_output=False, consume=True, stream=stream, share_with=base)
            m.setup(cases.lockstep_events(16, cases.LOCKSTEP_CLASSES[c], c), sync_interval=FLUSH)
            chains.append(m)
        image = capi.DeviceArray(np.eye(w.nparameters).reshape(-1))
        chains[1].group.SetConstraintWhitening(image)
        ls = LockstepChains(chains)
        with pytest.raises(capi.SxmcError) as e:
            ls.step()
        assert e.value.code == capi.ERR_STATE and "constraint whitening" in e.value.msg and "lockstep" in e.value.msg
        chains[1].group.SetConstraintWhitening(None)
        ls.step()
        capi.synchronize()
    finally:
        if ls is not None:
            ls.close()
        for m in chains[::-1]:
            close(m)
        close(base)
