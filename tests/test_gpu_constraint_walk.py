"""Whole walks with correlated constraints: mcmc.MCMC.walk(constraint_correlation=...) over a small fit with floating
systematics (tests/step_replay_cases.py, "c3/255": a shift, a scale and a resolution, whose three constraints are tied by
a dense correlation matrix), 600 steps with burn-in 0.2, so both re-tunings fall inside.

(a) One walk is FOLLOWED step by step by the host replay (tests/step_reference_constraints.py): every pending proposal
    within the project's bound on a device normal, the NLL against the oracle's with the whitened constraint terms, and
    from those the replay's decisions, rows, counters and generator offsets bit for bit, through both re-tunings.
(b) The free-running forms of the same walk -- eager, replayed from graphs of 16 steps, asked with lookahead (which such
    a walk answers by walking sequentially: no pass is launched) -- give the followed chain's bytes; and so they do among
    each other with the covariance proposal, with event weights and with a weighted histogram member.
(c) In every one of these W = I walks the chain of no matrix at all, as bytes, and the correlated chain is another one.
(d) The refusals: a matrix that is not one, the lockstep runner by name."""
import copy

import numpy as np
import pytest

from sxmc_amd import capi, ensemble
from sxmc_amd.mcmc import MCMC
from tests import step_reference_constraints as sc
from tests import step_replay_cases as cases
from tests.test_gpu_constraint_forms import ReplayConstrained
from tests.test_gpu_step_end_arith import bits

pytestmark = pytest.mark.gpu

NAME, SEED = "c3/255", 5
NSTEPS, BURNIN, SYNC = 600, 0.2, 150
MIN_MARGIN = 1e-4


def close(m):
    capi.synchronize()
    if m._graph is not None:
        m._graph.close()
    for p in m.pdfs:
        p.close()
    m.group.close()


def workload():
    return cases.workload_cached(NAME)


def rho_of(w, law):
    if law == "none":
        return None
    P = w.nparameters
    if law == "identity":
        return np.eye(P)
    idx = np.flatnonzero(w.parameter_sigmas() > 0)
    assert idx.size == 3
    return sc.block_matrix(P, [(idx, [[1.0, -0.6, 0.3], [-0.6, 1.0, 0.2], [0.3, 0.2, 1.0]])])


_followed = {}


def followed():
    """The consuming walk under the correlated law, launched step by step beside the replay.  Returns (chain,
    accepted); computed once, shared, never modified."""
    if "chain" in _followed:
        return _followed["chain"]
    w = workload()
    m = MCMC(w, seed=SEED, lut_output=False, consume=True, stream=capi.new_stream())
    try:
        m.walk_begin(w.events, NSTEPS, BURNIN, sync_interval=SYNC, constraint_correlation=rho_of(w, "correlated"))
        P = w.nparameters
        W = m.ConstraintWhitening()
        assert bits(W).tobytes() == bits(sc.whitening(rho_of(w, "correlated"))).tobytes()
        r = ReplayConstrained(m, w, SEED, SYNC, W)
        b = int(NSTEPS * BURNIN)
        for i in range(NSTEPS):
            if i in (b, 2 * b):
                kept = np.concatenate(m._rows, axis=0)
                assert kept.shape == (b, P + 1)
                pending = m.proposed_vector.get()
                m._retune_if_due(i)
                r.ref.retune(kept)
                jw = m.jump_width.get()
                assert np.allclose(jw, r.ref.jump_width, rtol=1e-6, atol=0), i
                r.ref.jump_width = jw.copy()
                r.width = np.clip(jw.astype(np.float64), 0.0, None)
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
        assert summary["rejections"] >= 20 and summary["accepted"] >= 20, summary
        assert chain.shape == (NSTEPS - 2 * b, P + 1)
        chain.setflags(write=False)
        _followed["chain"] = (chain, accepted)
    finally:
        close(m)
    return _followed["chain"]


def weighted_member(w):
    """w with multiplicities 1 + i % 3 on signal 1: a weighted histogram member."""
    w2 = copy.copy(w)
    w2.signals = list(w.signals)
    s = copy.copy(w.signals[1])
    s.multiplicities = (1 + np.arange(s.samples.shape[0]) % 3).astype(np.uint32)
    w2.signals[1] = s
    return w2


def walked(w, law, graph_steps=0, lookahead=False, **kw):
    m = MCMC(w, seed=SEED, lut_output=False, consume=True, stream=capi.new_stream())
    try:
        chain, accepted = m.walk(w.events, NSTEPS, BURNIN, sync_interval=SYNC, graph_steps=graph_steps,
                                 lookahead=lookahead, constraint_correlation=rho_of(w, law), **kw)
        assert m.lookahead_passes == 0
        if law != "none":
            assert not m.group.LookaheadSupported()
        return chain.tobytes(), accepted
    finally:
        close(m)


def test_walk_follows_the_host_replay_through_both_retunings():
    chain, accepted = followed()
    assert 0 < accepted < NSTEPS


SETTINGS = {"diagonal": {}, "covariance": dict(proposal="covariance"), "event weights": "weights",
            "sample weights": "member"}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_eager_graphs_and_lookahead_walk_one_chain_and_identity_is_no_matrix(setting):
    w = workload()
    kw = SETTINGS[setting]
    if kw == "weights":
        kw = dict(event_weights=0.25 * (1 + np.arange(w.events.shape[0]) % 7))
    elif kw == "member":
        w, kw = weighted_member(w), {}
    out = {}
    for law in ("none", "identity", "correlated"):
        eager = walked(w, law, **kw)
        if law != "none":
            assert walked(w, law, graph_steps=16, lookahead=True, **kw) == eager, (setting, law)
        if law == "correlated":
            assert walked(w, law, graph_steps=16, **kw) == eager, (setting, law)
            assert walked(w, law, lookahead=True, **kw) == eager, (setting, law)
        out[law] = eager
    assert out["identity"] == out["none"], setting
    assert out["correlated"][0] != out["none"][0], setting
    assert 0 < out["correlated"][1] < NSTEPS
    if setting == "diagonal":
        chain, accepted = followed()
        assert out["correlated"] == (chain.tobytes(), accepted)


def test_a_matrix_that_is_refused_says_why_and_leaves_the_chain_usable():
    w = workload()
    P = w.nparameters
    m = MCMC(w, seed=SEED, lut_output=False, consume=True, stream=capi.new_stream())
    try:
        bad = np.eye(P)
        bad[P - 1, P - 2] = bad[P - 2, P - 1] = 1.0
        with pytest.raises(capi.SxmcError, match="not positive definite at parameter %d" % (P - 1)):
            m.walk(w.events, 40, BURNIN, constraint_correlation=bad)
        bad = np.eye(P)
        bad[0, P - 1] = bad[P - 1, 0] = 0.5                       # rate 0 carries no constraint
        with pytest.raises(capi.SxmcError, match="parameter 0 has no constraint"):
            m.walk(w.events, 40, BURNIN, constraint_correlation=bad)
        with pytest.raises(ValueError, match="%d x %d" % (P, P)):
            m.walk(w.events, 40, BURNIN, constraint_correlation=np.eye(P - 1))
        chain, _ = m.walk(w.events, 40, BURNIN, sync_interval=40)
        assert chain.shape[0] == 40 - 2 * int(40 * BURNIN)
    finally:
        close(m)
    with pytest.raises(ValueError, match="lockstep sets have no step end with correlated constraints"):
        ensemble.run_experiments_in_lockstep(w, [1, 2], 40, [], constraint_correlation=np.eye(P))
