"""Whole walks with the correlated proposal: mcmc.MCMC.walk(proposal="covariance") over a small fit with floating
systematics, 600 steps with burn-in 0.2, so both re-tunings fall inside.

(a) One walk is FOLLOWED step by step by the host replay (tests/step_reference_cov.py), the way
    tests/test_gpu_step_replay.py and tests/test_gpu_step_end_arith.py follow the diagonal walk: every pending proposal
    within the bound of tests/test_gpu_proposal_forms.py's ReplayCov, the NLL against the oracle's, and from those the
    replay's decisions, rows, counters and generator offsets bit for bit.  At each re-tuning the replay is handed the rows
    the device kept and the widths the walk made of them, and its factor must be the walk's BYTES (the walk's comes from
    sxmc_proposal_factor through ctypes, the replay's from its own re-tuning).
(b) The free-running forms of the same walk -- eager, replayed from graphs of 16 steps, asked with lookahead (which a
    correlated walk answers by walking sequentially) -- give the followed chain's bytes.
(c) The forms whose NLL rounds differently (the reference's launches, the batched form, the experimental one-kernel step
    end) decide every step as the followed chain did and stay within the float store of it.
(d) A diagonal walk after a correlated one on the same object is the diagonal walk of a fresh object.
"""
import numpy as np
import pytest

from sxmc_amd import capi
from sxmc_amd.mcmc import MCMC
from tests import step_reference_cov as cov
from tests import step_replay_cases as cases
from tests.test_gpu_proposal_forms import ReplayCov
from tests.test_gpu_step_end_arith import bits

pytestmark = pytest.mark.gpu

# the seed: the first of 1 .. 8 whose replay on the host alone (replay_walk_cov with the oracle's NLL, no device) refuses
# and accepts uphill at least 20 steps each, the conditions of tests/step_replay_cases.py (seed 5: 470 refused, 26
# accepted uphill, smallest margin 0.023)
NAME, SEED = "c3/255", 5
NSTEPS, BURNIN, SYNC, SHRINKAGE = 600, 0.2, 150, 0.05
MIN_MARGIN = 1e-4            # (tests/step_replay_cases.py: no decision so close that an NLL's rounding could move it)


def close(m):
    capi.synchronize()
    if m._graph is not None:
        m._graph.close()
    for p in m.pdfs:
        p.close()
    m.group.close()


def new_walker(seed=SEED, **kw):
    w = cases.workload_cached(NAME)
    return w, MCMC(w, seed=seed, **kw)


_followed = {}


def followed(fixed=()):
    """The consuming walk over event classes, launched step by step beside the replay.  Returns (chain, accepted, the
    replay's decisions, the factors of the walk's three stretches); computed once, shared, never modified.
    fixed: parameters that do not float (width -1: they draw nothing, their z is 0 in every product behind them)."""
    if fixed in _followed:
        return _followed[fixed]
    w, m = new_walker(lut_output=False, consume=True, stream=capi.new_stream())
    if fixed:
        widths = MCMC.initial_jump_widths(m, [i in fixed for i in range(w.nparameters)])
        m.initial_jump_widths = lambda _fixed=None: widths.copy()
    try:
        m.walk_begin(w.events, NSTEPS, BURNIN, sync_interval=SYNC, proposal="covariance", proposal_shrinkage=SHRINKAGE)
        P = w.nparameters
        L0, used0 = m.ProposalFactor()
        assert used0 == SHRINKAGE and np.array_equal(L0, cov.diagonal_factor(m.jump_width.get()))
        r = ReplayCov(m, w, SEED, SYNC, L0)
        r.ref.shrinkage = SHRINKAGE
        factors = [L0]
        b = int(NSTEPS * BURNIN)
        for i in range(NSTEPS):
            if i in (b, 2 * b):
                kept = np.concatenate(m._rows, axis=0)
                assert kept.shape == (b, P + 1)
                pending = m.proposed_vector.get()
                m._retune_if_due(i)
                # the widths: the walk's own law, as before this change (double spread, one float rounding)
                r.ref.retune(kept)
                jw = m.jump_width.get()
                assert np.allclose(jw, r.ref.jump_width, rtol=1e-6, atol=0), i
                r.ref.jump_width = jw.copy()
                want, _, _, used = cov.retune_factor(kept, jw, SHRINKAGE)
                L, got_used = m.ProposalFactor()
                assert got_used == used == SHRINKAGE, (got_used, used)
                assert bits(L).tobytes() == bits(want).tobytes(), i
                assert np.count_nonzero(np.tril(L, -1)) > 0
                r.ref.factor = want
                r.width = np.clip(jw.astype(np.float64), 0.0, None)
                r.L = np.maximum(r.L, np.abs(want))
                factors.append(L)
                # the proposal already drawn stands
                assert np.array_equal(bits(m.proposed_vector.get()), bits(pending))
            r.before()
            m.step(False)
            capi.synchronize()
            assert m.group.StepEndTimeouts() == 0
            r.after(r.vp, i % 16 == 0)
            m._flush_if_due(i)
            if m._since_flush == 0:
                r.flushed()
        chain, accepted = m.walk_end()
        summary = r.ref.summary()
        print("followed walk:", summary)
        assert summary["min_margin"] >= MIN_MARGIN, summary
        if not fixed:      # (the seed was chosen for the walk with every parameter floating)
            assert summary["rejections"] >= 20 and summary["uphill_accepted"] >= 20, summary
        assert summary["rejections"] >= 1 and summary["accepted"] >= 1, summary
        assert chain.shape == (NSTEPS - 2 * b, P + 1)
        chain.setflags(write=False)
        _followed[fixed] = (chain, accepted, [d["accept"] for d in r.ref.decisions], factors)
    finally:
        close(m)
    return _followed[fixed]


def test_walk_follows_the_host_replay_through_both_retunings():
    chain, accepted, decisions, factors = followed()
    assert accepted == sum(decisions) and len(decisions) == NSTEPS and len(factors) == 3
    # the second factor differs from the first: each re-tuning rebuilt it from its own rows
    assert not np.array_equal(factors[1], factors[2])


def test_walk_with_fixed_parameters_follows_the_host_replay():
    """Rates 1 and 5 and the second systematic fixed, free parameters behind each: their columns of the chain never move,
    their rows and columns of every factor are zero, and the walk is the replay's through both re-tunings."""
    w = cases.workload_cached(NAME)
    fixed = (1, 5, w.nparameters - 2)
    chain, accepted, decisions, factors = followed(fixed)
    means = w.parameter_means().astype(np.float32)
    for j in fixed:
        assert np.all(chain[:, j] == means[j])
        for L in factors:
            assert np.all(L[j, :] == 0.0) and np.all(L[:, j] == 0.0)
    assert np.unique(chain[:, 2]).size > 1 and np.unique(chain[:, w.nparameters - 1]).size > 1
    assert np.count_nonzero(np.tril(factors[2], -1)) > 0


@pytest.mark.parametrize("graph_steps,lookahead", [(0, False), (16, False), (0, True), (16, True)])
def test_free_running_forms_walk_the_followed_chain(graph_steps, lookahead):
    want, want_accepted, _, factors = followed()
    w, m = new_walker(lut_output=False, consume=True, stream=capi.new_stream())
    try:
        chain, accepted = m.walk(w.events, NSTEPS, BURNIN, sync_interval=SYNC, graph_steps=graph_steps,
                                 lookahead=lookahead, proposal="covariance", proposal_shrinkage=SHRINKAGE)
        assert m.lookahead_passes == 0                          # asked with lookahead, a correlated walk goes step by step
        assert graph_steps == 0 or m._graph is not None
        L, used = m.ProposalFactor()
    finally:
        close(m)
    assert accepted == want_accepted
    assert bits(chain).tobytes() == bits(want).tobytes()
    assert bits(L).tobytes() == bits(factors[2]).tobytes() and used == SHRINKAGE


@pytest.mark.parametrize("form", ["reference", "fused", "step", "consume"])
def test_other_forms_decide_as_the_followed_chain(form):
    """Their NLL is the same sum in another order: every decision is the followed chain's (its margins say no rounding of
    an NLL moves one), the rows agree to the float they are stored as -- the re-tunings see rows that may differ in that
    last bit, which moves a factor by parts in 1e7 -- and the NLL column to the project's 1e-6."""
    want, want_accepted, decisions, _ = followed()
    if form == "consume":
        w, m = new_walker(lut_output=True, consume=True, stream=capi.new_stream())
    else:
        w, m = new_walker(fused={"reference": False, "fused": True, "step": "step"}[form])
    try:
        chain, accepted = m.walk(w.events, NSTEPS, BURNIN, sync_interval=SYNC, proposal="covariance",
                                 proposal_shrinkage=SHRINKAGE)
    finally:
        close(m)
    assert accepted == want_accepted and chain.shape == want.shape
    b = int(NSTEPS * BURNIN)
    repeated = np.all(bits(chain[1:]) == bits(chain[:-1]), axis=1)
    assert np.array_equal(repeated, ~np.array(decisions[2 * b + 1:]))
    P = chain.shape[1] - 1
    got64, want64 = chain.astype(np.float64), np.asarray(want, np.float64)
    # a step moves parameter i by (L z)_i, |z| < 6.7: the deviates agree to 8e-12, and a factor built from rows that
    # differ in their last float bit (2^-23 relative in a correlation) differs by at most 1 / shrinkage times that in T
    # (the shrunk matrix's smallest eigenvalue is the shrinkage); the differences add up over the steps at worst
    *_, factors = followed()
    reach = np.max([np.abs(L).sum(axis=1) for L in factors], axis=0)
    steps = np.arange(2 * b, NSTEPS)[:, None] + 1
    tol = 2.0 ** -24 * np.abs(want64[:, :P]) + steps * 6.7 * (8e-12 + 2.0 ** -23 / SHRINKAGE) * reach
    assert np.all(np.abs(got64[:, :P] - want64[:, :P]) <= tol)
    assert np.all(np.abs(got64[:, P] - want64[:, P]) <= 1e-6 * np.abs(want64[:, P]))


def test_a_diagonal_walk_after_a_correlated_one_is_the_diagonal_walk():
    w, fresh = new_walker(lut_output=False, consume=True, stream=capi.new_stream())
    try:
        want = fresh.walk(w.events, 200, BURNIN, sync_interval=SYNC, graph_steps=16)
        assert fresh.ProposalFactor() == (None, None)
    finally:
        close(fresh)
    w, m = new_walker(lut_output=False, consume=True, stream=capi.new_stream())
    try:
        m.walk(w.events, 200, BURNIN, sync_interval=SYNC, graph_steps=16, proposal="covariance")
        m.reseed(SEED)
        got = m.walk(w.events, 200, BURNIN, sync_interval=SYNC, graph_steps=16)
        assert m.ProposalFactor() == (None, None)
    finally:
        close(m)
    assert got[1] == want[1] and bits(got[0]).tobytes() == bits(want[0]).tobytes()


def test_walk_refuses_what_it_cannot_mean():
    w, m = new_walker()
    try:
        with pytest.raises(ValueError, match="diagonal.*covariance"):
            m.walk(w.events, 10, 0.2, proposal="haario")
        for bad in (0.0, -1.0, 1.5):
            with pytest.raises(ValueError, match=r"\(0, 1\]"):
                m.walk(w.events, 10, 0.2, proposal="covariance", proposal_shrinkage=bad)
    finally:
        close(m)
