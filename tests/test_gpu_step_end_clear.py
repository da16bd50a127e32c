"""The clearing at the end of a step (clear_piece, sxmc_amd/csrc/step_end_kernels.inc.h) at the edges of its index
arithmetic: 16-byte stores over n >> 2 words of four, chunk 0 clearing the n & 3 words behind them.  Every other
step-end case of the suite has a bin count that is a multiple of 4; here

    1 x 3    n4 = 0: nothing but the tail          1 x 5     one store and one tail word
    7 x 9    63 = 15 * 4 + 3                       23 x 23   529 words: 132 stores -- two chunks of 128 lanes -- and one

in every form that clears, where the host's rules offer the form for the shape (each test asserts WHICH FORM RAN, from
the launches behind the fill, as tests/test_gpu_step_end_forms.py does):

    zero          zero_kernel: a second evaluation over the first one's counts
    two           eval_nll_kernel + finish_zero_kernel (cooperative and one-workgroup ends switched off)
    tail          tail_step_kernel: 4 to 41 event classes x 2 members, at most 256 look-ups
    coop          step_end_kernel: rows are the 300 events (lookup table on), 600 look-ups
    lookahead-two eval_nll2_kernel + finish2_zero_kernel, both groups' histograms
    lookahead-coop step_end2_kernel, both groups' histograms
    joint         eval_nll_chains_kernel + finish_zero_chains_kernel, two chains (rows are the events: chain by chain
                  each end would be cooperative, one launch; the set's two launches are the joint form)

LEFT OUT: lookahead-coop at 1 x 3, 1 x 5 and 7 x 9.  The pass is refused where the sequential step would end in one
workgroup, and two members over at most 64 classes are at most 128 look-ups; with that form switched off (which is how
`two`, `lookahead-two` and `joint` run at these shapes) the host offers no cooperative end either.  It runs at 23 x 23
(201 classes, 402 look-ups).  The fused step (fill_step_kernel) clears through the same step_end_role as `coop` and
needs an ordered table; tests/test_gpu_step_end_forms.py walks it.

Two members of 4 000 and 4 500 samples, flat over the whole box (so that the LAST words of every histogram -- the tail,
the second chunk -- hold counts at every vector of the walk: asserted from the oracle), 300 events.  Eight steps are walked and flushed (no wait gave up); then the group's
histograms are evaluated once more, at a fixed vector -- through the pre-zeroed path: the step end's clearing is all
that stands between the walk's counts and this evaluation's -- and every member's COUNTS are compared, exactly, with
the CPU oracle's for that vector.  The reference is the oracle, not another form: every form clears through one function.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, workloads
from sxmc_amd.mcmc import MCMC, LockstepChains, LookaheadWalk
from tests.test_gpu_step_end_arith import close
from tests.test_gpu_step_end_forms import ONE_LAUNCH, TWO_LAUNCHES, fills, new_chain
from tests.test_gpu_step_end_table import HI, LO, make_events

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (1, 5), (7, 9), (23, 23)]
NSTEPS, NEVENTS = 8, 300


@functools.lru_cache(maxsize=None)
def workload(nbins, few):
    """Built once per shape, shared, never modified.  `few`: as few event classes as the one-workgroup end takes."""
    rng = np.random.default_rng(29)
    signals = []
    for j in range(2):
        # over the WHOLE box, a few to every bin of the finest shape: the words at the end of a histogram -- the n & 3
        # tail, the second chunk -- are counted at every vector of the walk (expected() asserts it), so a clearing that
        # skipped them would show.  (The first observable is flat to beyond the upper edge: the scale systematic moves
        # samples across it both ways.)
        n = 4000 + 500 * j
        e = rng.uniform(0.0, 10.6, size=n)
        r = rng.uniform(0.0, 6.0, size=n)
        tab = np.stack([e, r, np.zeros(n)], axis=1).astype(np.float32)
        signals.append(workloads.Signal(tab, 3, nexpected=60.0 + 7 * j, source_id=j))
    nb = nbins[0] * nbins[1]
    classes = min(nb, 40 if few else 200) + 1
    ev = make_events(rng, nbins, classes, NEVENTS)
    w = workloads.Workload("clear", 2, LO, HI, list(nbins), signals, [dict(type="scale", obs=0, pars=[0])], [0.01], ev,
                           "%d x %d bins, %d event classes" % (nbins[0], nbins[1], classes))
    w.classes = classes
    return w


@functools.lru_cache(maxsize=None)
def expected(nbins):
    """The fixed vector and the oracle's counts of both members at it: computed once per shape, never modified."""
    w = workload(nbins, False)
    vec = w.parameter_means().astype(np.float64).copy()
    vec[w.nsources:] += 0.02
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    n = nbins[0] * nbins[1]
    # the words a faulty clearing could leave: the n & 3 behind the last 16-byte store, and everything beyond the first
    # chunk of 128 lanes x 4 words (finish_zero_kernel's, step_end_kernel's and step_end2_kernel's workgroups)
    edge = sorted(set(range(n - (n & 3), n)) | set(range(4 * 128, n)))
    assert edge and (n < 512 or edge[0] == 512), edge
    counts = []
    for s in w.signals:
        # dirty at every vector the walk can hold (the systematic's sigma is 0.01) ...
        for shift in (-0.05, -0.03, -0.01, 0.0, 0.01, 0.03, 0.05):
            at = vec[w.nsources:] - 0.02 + shift
            dirty = np.asarray(oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, at)[0])
            assert np.all(dirty[edge] > 0), (nbins, shift, dirty[edge])
        # ... and counted at the fixed one
        bins, norm = oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, vec[w.nsources:])
        bins = np.asarray(bins, np.uint32).copy()
        assert bins.size == n and int(bins.sum()) == int(norm) > 100 and np.all(bins[edge] > 0), bins[edge]
        bins.setflags(write=False)
        counts.append(bins)
    vec.setflags(write=False)
    return vec, counts


def check_cleared(m, nbins):
    """One more evaluation of m's group, at the fixed vector, over what the step end left: the oracle's counts."""
    vec, want = expected(nbins)
    capi.synchronize()
    m.proposed_vector.set(vec)
    m.group.EvalAsync(False, m.stream)
    capi.synchronize()
    for j, p in enumerate(m.pdfs):
        got = p.GetBins()
        assert np.array_equal(got, want[j]), (j, np.argwhere(got != want[j])[:4].ravel(), got[-4:], want[j][-4:])


def flushed(m):
    m.flush()
    assert m.group.StepEndTimeouts() == 0


def sequential(nbins, end, lookups, **kw):
    """Eight steps of one chain, ended as `end` says; `lookups`: which side of the one-workgroup end's 256 the shape is."""
    few = kw.pop("few", False)
    w = workload(nbins, few)
    rows = NEVENTS if kw.get("lut_output") else w.classes
    assert lookups(rows * w.nsignals), (rows, w.nsignals)
    m = new_chain(w, **kw)
    try:
        m.step()
        m.steps(NSTEPS - 1)
        flushed(m)
        assert m.group.LastStepLaunches() - fills(m) == end, (m.group.LastStepLaunches(), m.group.LaunchInfo())
        check_cleared(m, nbins)
    finally:
        close(m)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_zero_kernel(nbins):
    w = workload(nbins, False)
    m = new_chain(w, coop=False, tail=False)
    try:
        capi.synchronize()
        m.proposed_vector.set(w.parameter_means().astype(np.float64))
        m.group.EvalAsync(False, m.stream)                         # (counts that the next evaluation's zero launch clears)
        check_cleared(m, nbins)
    finally:
        close(m)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_two_launch_end(nbins):
    sequential(nbins, TWO_LAUNCHES, lambda n: True, coop=False, tail=False)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_one_workgroup_end(nbins):
    sequential(nbins, ONE_LAUNCH, lambda n: n <= 256, coop=False, tail=True, few=True)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_cooperative_end(nbins):
    sequential(nbins, ONE_LAUNCH, lambda n: n > 256, coop=True, tail=True, lut_output=True)


def lookahead(nbins, coop, tail, end):
    w = workload(nbins, False)
    m = new_chain(w, coop=coop, tail=tail)
    la = None
    try:
        assert m.group.LookaheadSupported()
        la = LookaheadWalk(m, threads=0)
        la.shadow.group.SetTailKernel(tail)
        la.bind(w.events)
        done = la.steps(1, count0=0)
        done = la.steps(NSTEPS - 1, count0=done)
        assert done == NSTEPS
        la.one_pass()                                              # (beyond the stop: decides nothing, clears again;
        la.one_pass()                                              #  the second has no zeroing launch in front of it)
        assert m.group.LastStepLaunches() - fills(m) == end
        flushed(m)
        check_cleared(m, nbins)
        check_cleared(la.shadow, nbins)
    finally:
        if la is not None:
            la.close()
        close(m)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_lookahead_two_launch_end(nbins):
    lookahead(nbins, False, False, TWO_LAUNCHES)


def test_lookahead_cooperative_end():
    nbins = (23, 23)
    assert workload(nbins, False).classes * 2 > 256
    lookahead(nbins, True, True, ONE_LAUNCH)


@pytest.mark.parametrize("nbins", SHAPES, ids=repr)
def test_joint_lockstep_ends(nbins):
    # (rows are the events, 600 look-ups: chain by chain every end would be cooperative, ONE launch -- two are the set's)
    w = workload(nbins, False)
    stream = capi.new_stream()
    base = MCMC(w, seed=1, lut_output=True, consume=True, stream=stream)
    chains, ls = [], None
    try:
        for c in range(2):
            chains.append(new_chain(w, lut_output=True, seed=5 + c, stream=stream, share_with=base))
        ls = LockstepChains(chains)
        ls.mg.SetJointStepEnd(True)
        for _ in range(NSTEPS):
            ls.step()
        for m in chains:
            flushed(m)
            assert m.group.LastStepLaunches() - fills(m) == TWO_LAUNCHES
        for m in chains:
            check_cleared(m, nbins)
    finally:
        if ls is not None:
            ls.close()
        for m in chains[::-1]:
            close(m)
        close(base)
