"""The cooperative step end with its look-up pointers by value (step_end_kernel<true>: groups of up to 16 members take
the rows' bin tables and the histograms as a kernel argument and gather before the staging barrier).  The descriptor
path -- the two-launch step end, and the cooperative one for more than 16 members -- is the built-in reference: same
virtual blocks, same arithmetic, so every chain must be the reference's bit for bit.  Kernel arguments are frozen into a
recorded graph, so whatever rebuilds the table (new evaluation points, another form of the fill) must be followed by
steps that see the new one, launched one by one or replayed."""
import numpy as np
import pytest

from sxmc_amd import capi, workloads
from sxmc_amd.mcmc import MCMC

pytestmark = pytest.mark.gpu

LO, HI = [0.0, 0.0], [10.0, 6.0]


def make_events(rng, nbins, nclasses, n):
    """`n` events in exactly `nclasses` classes: nclasses - 1 distinct bins (their centres, random multiplicities) and,
    where there is more than one class, events outside the histogram (bin -2 in every member)."""
    nb = nbins[0] * nbins[1]
    inside = max(1, nclasses - 1)
    cells = rng.choice(nb, size=inside, replace=False)
    pick = np.concatenate([cells, rng.choice(cells, size=n - inside - (8 if nclasses > 1 else 0))])
    ev = np.zeros((n, 3), np.float32)
    k = pick.size
    ev[:k, 0] = (pick // nbins[1] + 0.5) * (HI[0] - LO[0]) / nbins[0]
    ev[:k, 1] = (pick % nbins[1] + 0.5) * (HI[1] - LO[1]) / nbins[1]
    ev[k:, 0] = 99.0                                         # outside every member
    ev[k:, 1] = 1.0
    return ev[rng.permutation(n)]


def make_workload(nsig, nclasses, nbins=(20, 20), seed=7, nevents=1500):
    """nsig small 2-D signals with a scale systematic; signals 1 and 2 share a source, and the last signal of a group of
    three or more has every sample outside the histogram (normalisation 0)."""
    rng = np.random.default_rng(seed)
    signals = []
    for j in range(nsig):
        n = 3000 + 100 * j
        e = rng.normal(3.0 + 0.3 * j, 1.5, size=n)
        r = 6.0 * rng.uniform(0.0, 1.0, size=n) ** (1.0 / 3.0)
        if nsig >= 3 and j == nsig - 1:
            e = e + 50.0
        tab = np.stack([e, r, np.zeros(n)], axis=1).astype(np.float32)
        source = j if j < 2 else j - 1                       # (signals 1 and 2: one source)
        signals.append(workloads.Signal(tab, 3, nexpected=60.0 + 7 * j, source_id=source))
    systs = [dict(type="scale", obs=0, pars=[0])]
    ev = make_events(rng, nbins, nclasses, nevents)
    return workloads.Workload("table", 2, LO, HI, list(nbins), signals, systs, [0.01], ev,
                              "S=%d, %d event classes" % (nsig, nclasses))


def close(m):
    capi.synchronize()
    if m._graph is not None:
        m._graph.close()
    for p in m.pdfs:
        p.close()
    m.group.close()


def new_chain(w, coop, seed=5):
    m = MCMC(w, seed=seed, lut_output=False, consume=True, stream=capi.new_stream())
    m.group.SetCooperativeStepEnd(coop)
    m.group.SetFusedStep(False)
    return m


def state(m):
    capi.synchronize()
    return (m.current_nll.get().view(np.uint64).copy(), m.proposed_nll.get().view(np.uint64).copy())


def walk(w, coop, nsteps, graph_steps=0):
    m = new_chain(w, coop)
    chain, acc = m.walk(w.events, nsteps, 0.1, sync_interval=50, graph_steps=graph_steps)
    out = (chain, acc, state(m), m.group.LastStepLaunches(), m.group.StepEndTimeouts())
    close(m)
    return out


# 20 x 20 bins: 300 classes are two full virtual blocks of 128 rows and a partial one.  One class: a histogram large
# enough (16 x 64 x 65 words) that the step end is not the one-workgroup form, which small problems take instead.
@pytest.mark.parametrize("nsig,nclasses,nbins", [(1, 300, (20, 20)), (12, 300, (20, 20)), (16, 300, (20, 20)),
                                                 (17, 300, (20, 20)), (16, 1, (64, 65))])
def test_table_step_end_walks_the_two_launch_chain(nsig, nclasses, nbins):
    w = make_workload(nsig, nclasses, nbins)
    want = walk(w, False, 64)
    assert want[3] >= 3 and want[4] == 0                      # fill + event sum + step end: the descriptor path
    for graph_steps in (0, 8):
        got = walk(w, True, 64, graph_steps)
        assert got[3] == want[3] - 1, got[3]                  # fill + ONE step-end launch
        assert got[4] == 0
        assert got[1] == want[1]
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1])
    if nsig >= 3:
        m = new_chain(w, True)
        m.setup(w.events, sync_interval=8)
        assert m.normalizations.get()[-1] == 0                # (the member whose samples all lie outside)
        close(m)


def steps16(m, graph_steps):
    m.step()                                                   # (one step launched directly before any is recorded)
    m.steps(15, graph_steps)


def rebind_walks(w, second, graph_steps):
    """16 steps on w.events, then `second` as the evaluation points, 16 more; and a fresh chain set up on `second` from
    the first one's state at that point.  Returns both second halves."""
    a = new_chain(w, True)
    a.setup(w.events, sync_interval=64)
    steps16(a, graph_steps)
    a.flush()
    vector, rngs = a.current_vector.get().copy(), a.rngs.get().copy()
    a.setup(second, sync_interval=64)
    steps16(a, graph_steps)
    rows_a, acc_a = a.flush()
    got = (rows_a, acc_a, state(a), a.group.StepEndTimeouts())
    close(a)

    b = new_chain(w, True)
    b.current_vector.set(vector)
    b.rngs.set(rngs)
    b.setup(second, sync_interval=64)
    steps16(b, graph_steps)
    rows_b, acc_b = b.flush()
    want = (rows_b, acc_b, state(b), b.group.StepEndTimeouts())
    close(b)
    return got, want


@pytest.mark.parametrize("graph_steps", [0, 4])
def test_new_evaluation_points_reach_the_step_end(graph_steps):
    """Other events and another count of them: the class tables move, and with them the pointers a recorded or a
    directly launched step end holds by value."""
    w = make_workload(12, 300)
    second = make_events(np.random.default_rng(99), (20, 20), 140, 900)
    got, want = rebind_walks(w, second, graph_steps)
    assert got[3] == 0 and want[3] == 0
    assert got[1] == want[1] and got[0].shape == (16, w.nparameters + 1)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1])


_dual = []


def dual_plan_workload():
    if not _dual:
        _dual.append(workloads.config3(0.25, nevents=5000))    # (the smallest table whose plan keeps both forms)
    return _dual[0]


@pytest.mark.parametrize("graph_steps", [0, 4])
def test_fill_form_switch_reaches_the_step_end(graph_steps):
    """A plan with a boxed and an ordered form of the fill: steps in one form, then in the other, through the same step
    end -- the same chain as a chain that only ever knew the second form."""
    w = dual_plan_workload()
    forms = []
    a = new_chain(w, True)
    a.setup(w.events, sync_interval=64)
    assert "boxed+codes|ordered+codes" in a.group.LaunchInfo()
    a._adapt_pending = False
    a.group.SetFillForm(2)
    steps16(a, graph_steps)
    capi.synchronize()
    a.group.SetFillForm(1)
    if a._graph is not None:                                   # (what flush() does when the form changes)
        a._graph.close()
        a._graph = None
    forms.append(a.group.FillForm())
    steps16(a, graph_steps)
    capi.synchronize()
    rows_a = a.jump_buffer.get()[: 32 * (w.nparameters + 1)].copy()
    got = (rows_a, state(a), a.group.StepEndTimeouts())
    close(a)

    b = new_chain(w, True)
    b.setup(w.events, sync_interval=64)
    b._adapt_pending = False
    b.group.SetFillForm(1)
    steps16(b, graph_steps)
    steps16(b, graph_steps)
    capi.synchronize()
    rows_b = b.jump_buffer.get()[: 32 * (w.nparameters + 1)].copy()
    want = (rows_b, state(b), b.group.StepEndTimeouts())
    close(b)
    assert forms == [1] and got[2] == 0 and want[2] == 0
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1])
