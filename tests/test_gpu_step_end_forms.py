"""Every way a Metropolis step can end BESIDES the sequential step end, at the edges the sequential one is tested at
(tests/test_gpu_step_end_table.py, tests/test_gpu_step_end_arith.py): they all call eval_nll_block_part and
finish_step_device_w with their own picture of the grid, their own block size and their own register budget.

  (a) the look-ahead pass (LookaheadWalk): cooperative (step_end2_kernel: 2 nvb polling lanes, the second decision from
      s_part + nvb, peek_next_proposal_device) and in two launches (eval_nll2_kernel's two halves, finish2_zero_kernel);
  (b) lockstep sets (LockstepChains): joint ends (eval_nll_chains_kernel / finish_zero_chains_kernel, chain = blockIdx.y,
      chains of 1, 3, 2 and 1 blocks in one grid) and chain by chain;
  (c) the one-workgroup end (tail_step_kernel: 1024 lanes, finish_step_device<8>) on both sides of its 256 look-ups and
      65 536 histogram words;
  (d) the whole step in one launch (fill_step_kernel: BD = 128, R = 8);
  (e) one case each of (a), (b) and (c) step by step beside the host replay (tests/step_reference.py) and the oracle.

THE REFERENCE of (a)-(d) is the project's two-launch sequential chain -- a fresh MCMC with SetCooperativeStepEnd(False),
SetFusedStep(False), SetTailKernel(False) over the same workload and seed -- and everything is compared as bit patterns
(record() / same() of tests/test_gpu_step_end_arith.py): jump-buffer rows, accept count, both NLLs, both vectors, the
generators.  64 steps, flushed twice; the first step launched directly, the rest eager, and again replayed from a graph of
8 steps or passes.  Every test asserts WHICH FORM RAN from the launches per step (LastStepLaunches() against the fill's
launches in LaunchInfo()) or from the refusal's text: a case that falls back to another form fails.

The cases and what the host's rules make of them: tests/step_end_form_cases.py, checked without a device by
tests/test_step_end_form_cases_cpu.py.  (e) keeps the bounds of test_phase_b_follows_the_host_replay: NLL_RTOL on an NLL,
the proposal bound of tests/test_gpu_step_replay.py on a device normal.
"""
import numpy as np
import pytest

from sxmc_amd import capi, nll
from sxmc_amd.mcmc import MCMC, LockstepChains, LookaheadWalk
from tests import step_end_form_cases as cases
from tests.test_gpu_step_end_arith import Replay, _Widths, bits, close, record, same

pytestmark = pytest.mark.gpu

SEED = 5
NSTEPS, FLUSH, GRAPH = 64, 32, 8
TWO_LAUNCHES, ONE_LAUNCH, IN_THE_FILL = 2, 1, 0          # step-end launches behind the fill's


def widths_of(case, w, fixed=None):
    """The walk's own widths; the workloads of hundreds of sources: 0.04 per rate (tests/test_gpu_step_end_arith.py,
    test_long_vectors_walk_the_two_launch_chain: the walk's own, shared among so many, barely move the NLL) and a fifth
    of its sigma for the systematic."""
    if case is not None and case.members > 100:
        jw = np.full(w.nparameters, 0.04, np.float32)
        jw[w.nsources:] = np.float32(0.002)
        return jw
    return MCMC.initial_jump_widths(_Widths(w), fixed)


def new_chain(w, coop=None, fused=False, tail=True, lut_output=False, jump_width=None, seed=SEED, stream=None,
              share_with=None, data=None, dense=False, ordering=False, prebinning=True, rows=FLUSH):
    m = MCMC(w, seed=seed, lut_output=lut_output, consume=True, stream=stream or capi.new_stream(), share_with=share_with)
    if coop is not None:
        m.group.SetCooperativeStepEnd(coop)
    m.group.SetFusedStep(fused)
    m.group.SetTailKernel(tail)
    if dense:
        m.group.SetSparse(False)
    if ordering:
        m.group.SetOrdering(True, force=True)              # (a table this small would not be ordered by default)
    if not prebinning:
        m.group.SetPrebinning(False)
    m.setup(w.events if data is None else data, sync_interval=rows, jump_width=jump_width)
    return m


def fills(m):
    """The launches of the chain's fill (one line of LaunchInfo() each)."""
    return sum(1 for line in m.group.LaunchInfo().splitlines() if line.startswith("launch "))


def walk(m, graph_steps, lut_output=False):
    """NSTEPS steps of chain m, flushed every FLUSH: the first step launched directly, the others one by one or replayed
    from a graph.  Returns the flushes' records, the lookup table's bits and the step-end launches behind the fill."""
    out, ends = [], set()
    for _ in range(0, NSTEPS, FLUSH):
        m.step()
        m.steps(FLUSH - 1, graph_steps)
        out.append(record(m))                                  # (flush(): raises if a workgroup gave up waiting)
        ends.add(m.group.LastStepLaunches() - fills(m))
        assert m.group.StepEndTimeouts() == 0
    lut = bits(m.lut.get()).copy() if lut_output else None
    return out, lut, ends


_reference = {}


def _frozen(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    return id(v) if isinstance(v, MCMC) else v


def reference(name, w, **kw):
    """The two-launch sequential chain over w: computed once per workload and set of switches (everything that shapes
    the chain is part of the key; a chain that shares another's tables is the same chain whichever it shares them with),
    shared, never modified."""
    key = (name, id(w)) + tuple((k, _frozen(v)) for k, v in sorted(kw.items()) if k != "share_with")
    if key not in _reference:
        lut_output = kw.get("lut_output", False)
        m = new_chain(w, coop=False, fused=False, tail=False, **kw)
        try:
            out, lut, ends = walk(m, 0, lut_output=lut_output)
        finally:
            close(m)
        assert ends == {TWO_LAUNCHES}, ends
        assert 0 < sum(r["nacc"] for r in out) < NSTEPS, [r["nacc"] for r in out]
        for r in out:
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _reference[key] = (out, lut)
    return _reference[key]


def all_same(got, want):
    assert len(got) == len(want) == NSTEPS // FLUSH
    for g, r in zip(got, want):
        same(g, r)


# ============================================================================================ (a) the look-ahead pass
def lookahead_walk(w, coop, graph_passes, pieces=None, jump_width=None, prebinning=True):
    """NSTEPS steps in look-ahead passes, flushed every FLUSH.  pieces: the steps of each flush cut into stops; by default
    one step (one pass launched directly), then the rest.  Returns records, end launches, passes, whether a graph ran.
    The form is read off two more passes at every flush, launched BEYOND the stop: they decide nothing -- the records
    are taken after them --, and the second has no zeroing launch in front of it (the first pass after a recording has)."""
    m = new_chain(w, coop=coop, jump_width=jump_width, prebinning=prebinning)
    la = None
    try:
        assert m.group.LookaheadSupported()
        la = LookaheadWalk(m, threads=0)
        if not prebinning:
            la.shadow.group.SetPrebinning(False)               # (the two sets of evaluators: one launch plan)
        la.bind(w.events)
        out, ends, replayed, passes = [], set(), False, 0
        for f in range(NSTEPS // FLUSH):
            done = 0
            for i, piece in enumerate(pieces[f] if pieces else (1, FLUSH - 1)):
                done = la.steps(piece, graph_passes=0 if f == 0 and i == 0 else graph_passes, count0=done)
            assert done == FLUSH
            replayed = replayed or la._graph is not None
            passes = la.passes - 2 * f
            la.one_pass()
            la.one_pass()
            ends.add(m.group.LastStepLaunches() - fills(m))
            out.append(record(m))
            assert m.group.StepEndTimeouts() == 0
        return out, ends, passes, replayed
    finally:
        if la is not None:
            la.close()
        close(m)


def check_lookahead(key, w, jump_width=None, pieces=None, forms=((True, ONE_LAUNCH), (False, TWO_LAUNCHES)),
                    prebinning=True, graphs=(0, GRAPH)):
    want, _ = reference(key, w, jump_width=jump_width, prebinning=prebinning)
    for coop, end in forms:
        for graph_passes in graphs:
            got, ends, passes, replayed = lookahead_walk(w, coop, graph_passes, pieces, jump_width, prebinning)
            assert ends == {end}, (coop, graph_passes, ends)
            assert replayed == (graph_passes > 0)
            print(key, "cooperative" if coop else "two launches", "graph", graph_passes, "passes", passes, "accepted",
                  sum(r["nacc"] for r in got))
            assert passes < NSTEPS, passes                     # rejections were decided two steps per pass
            all_same(got, want)


@pytest.mark.parametrize("case", cases.LOOKAHEAD, ids=repr)
def test_lookahead_walks_the_two_launch_chain(case):
    """1 / 12 / 16 / 17 members, 127 / 128 / 129 / 300 classes: both ends of the pass."""
    check_lookahead(repr(case), case.workload())


def test_lookahead_at_the_worker_limit():
    """8 192 classes: 64 blocks per candidate, all 128 lanes of the finisher poll."""
    case = cases.WORKERS_AT_LIMIT
    check_lookahead(repr(case), case.workload(), prebinning=case.prebinning)


def test_lookahead_beyond_the_worker_limit_ends_in_two_launches():
    """8 193 classes: 65 blocks per candidate -- the two-launch end whatever the switch says."""
    case = cases.WORKERS_BEYOND
    check_lookahead(repr(case), case.workload(), forms=((True, TWO_LAUNCHES), (False, TWO_LAUNCHES)),
                    prebinning=case.prebinning)


def test_lookahead_in_odd_pieces():
    """Stops after 17, 1, 2, ... steps, honoured exactly -- and, asserted from the chain's own decisions, reached both by an
    A-step (also where the stop allowed two steps) and by a B-step."""
    case = cases.LOOKAHEAD[5]
    assert (case.members, case.classes) == (17, 300)
    w = case.workload()
    check_lookahead(repr(case), w, pieces=cases.PIECES)
    # the chain's decisions (a refused step repeats the row before it) say which step of a pass reached each stop
    want, _ = reference(repr(case), w, jump_width=None, prebinning=True)
    rows = np.concatenate([r["rows"].reshape(r["count"], w.nparameters + 1) for r in want])
    start = bits(w.parameter_means().astype(np.float32))
    accepted = [not np.array_equal(rows[k, :-1], rows[k - 1, :-1] if k else start) for k in range(NSTEPS)]
    assert sum(accepted) == sum(r["nacc"] for r in want)
    reached = cases.stops_reached_by(accepted, cases.PIECES[0] + cases.PIECES[1])
    print("stops reached by", reached)
    assert "A" in reached[1:] and "B" in reached, reached
    assert any(a == "A" and p > 1 for a, p in zip(reached, cases.PIECES[0] + cases.PIECES[1])), reached


def test_lookahead_with_parameter_0_and_a_systematic_fixed():
    """finish_step_device_w draws generator 0's uniform also when parameter 0 is fixed; peek_next_proposal_device must
    agree with it (and draw no deviate for either fixed parameter)."""
    case = cases.FIXED
    w = case.workload()
    fixed = [i == 0 or i == w.nparameters - 1 for i in range(w.nparameters)]
    jw = widths_of(case, w, fixed)
    assert jw[0] == -1 and jw[-1] == -1 and np.count_nonzero(jw > 0) == w.nparameters - 2
    check_lookahead(repr(case) + " fixed", w, jump_width=jw)
    want, _ = reference(repr(case) + " fixed", w, jump_width=jw, prebinning=True)
    means = w.parameter_means().astype(np.float32)
    for r in want:                                             # (the fixed parameters never moved)
        rows = r["rows"].view(np.float32).reshape(r["count"], w.nparameters + 1)
        assert np.all(rows[:, 0] == means[0]) and np.all(rows[:, w.nparameters - 1] == means[-1])
        assert np.unique(rows[:, 1]).size > 1


@pytest.mark.parametrize("graph_passes", [0, GRAPH])
@pytest.mark.parametrize("coop,end", [(True, ONE_LAUNCH), (False, TWO_LAUNCHES)])
def test_lookahead_with_256_parameters(coop, end, graph_passes):
    """The most the pass stages: both ends, eager and replayed (a case each: hundreds of evaluators take a second or two
    to set up, and every walk needs two sets of them)."""
    case = cases.PARAMETERS_256
    w = case.workload()
    assert w.nparameters == 256 and w.nsignals == 255
    check_lookahead(repr(case), w, jump_width=widths_of(case, w), forms=((coop, end),), graphs=(graph_passes,))


def refused(w, jump_width=None):
    m = new_chain(w, jump_width=jump_width)
    la = LookaheadWalk(m, threads=0)
    try:
        la.bind(w.events)
        supported = m.group.LookaheadSupported()
        with pytest.raises(capi.SxmcError) as err:
            la.one_pass()
        return supported, str(err.value)
    finally:
        la.close()
        close(m)


def test_lookahead_refuses_257_parameters():
    case = cases.PARAMETERS_257
    w = case.workload()
    assert w.nparameters == 257
    _, text = refused(w, widths_of(case, w))
    assert "at most 256 parameters" in text, text


def test_lookahead_refuses_a_shape_of_the_one_workgroup_end():
    case = cases.TAIL_TAKEN[0]
    supported, text = refused(case.workload())
    assert not supported and "not offered for this shape" in text, text


# ============================================================================================ (b) lockstep sets
def alone(w, members, classes, chain, base):
    """Chain `chain` of a set walked alone, in the two-launch sequential form."""
    ev = cases.lockstep_events(members, classes, chain)
    return reference(("alone", members, classes, chain), w, seed=SEED + chain, share_with=base, data=ev)[0]


def lockstep_walk(members, classes, joint, graph_steps):
    """The set of len(classes) chains over shared tables, NSTEPS steps flushed every FLUSH.  Returns every chain's records,
    the references and the step-end launches behind the fill seen by each chain."""
    w = cases.lockstep_workload(members)
    base = MCMC(w, seed=1, lut_output=False, consume=True, stream=capi.new_stream())
    chains, ls = [], None
    try:
        want = [alone(w, members, k, c, base) for c, k in enumerate(classes)]
        stream = capi.new_stream()
        for c, k in enumerate(classes):
            chains.append(new_chain(w, seed=SEED + c, stream=stream, share_with=base,
                                    data=cases.lockstep_events(members, k, c)))
        ls = LockstepChains(chains)
        ls.mg.SetJointStepEnd(joint)
        got, ends = [[] for _ in chains], [set() for _ in chains]
        for _ in range(NSTEPS // FLUSH):
            ls.step()                                          # (the first step is launched; recording needs the plans)
            ls.steps(FLUSH - 1, graph_steps)
            for c, m in enumerate(chains):
                got[c].append(record(m))
                ends[c].add(m.group.LastStepLaunches() - fills(m))
                assert m.group.StepEndTimeouts() == 0
        return got, want, ends
    finally:
        if ls is not None:
            ls.close()
        for m in chains[::-1]:
            close(m)
        close(base)


@pytest.mark.parametrize("nchains,joint", cases.LOCKSTEP_SETS)
@pytest.mark.parametrize("members", cases.LOCKSTEP_MEMBERS)
def test_lockstep_chains_of_very_different_sizes(members, nchains, joint):
    """40 / 300 / 129 / 128 classes: 1, 3, 2 and 1 blocks, so that most of the joint grid returns at once -- and every
    chain is the chain it walks alone.  2, 3 and 4 chains, joint ends and chain by chain, eager and replayed."""
    classes = cases.LOCKSTEP_CLASSES[:nchains]                 # (1 block beside 3; 1, 3, 2; 1, 3, 2, 1)
    for graph_steps in (0, GRAPH):
        got, want, ends = lockstep_walk(members, classes, joint, graph_steps)
        for c in range(nchains):
            # joint: the set's two launches; chain by chain: every chain's own cooperative step end
            assert ends[c] == {TWO_LAUNCHES if joint else ONE_LAUNCH}, (graph_steps, c, ends)
            all_same(got[c], want[c])


@pytest.mark.parametrize("members", cases.LOCKSTEP_MEMBERS)
def test_lockstep_set_with_a_chain_of_the_one_workgroup_end(members):
    """One chain small enough for tail_step_kernel: joint ends are asked for, the ends go chain by chain."""
    classes = [300, cases.LOCKSTEP_SMALL, 129]
    for graph_steps in (0, GRAPH):
        got, want, ends = lockstep_walk(members, classes, True, graph_steps)
        for c in range(3):
            assert ends[c] == {ONE_LAUNCH}, (c, ends)
            all_same(got[c], want[c])


def test_lockstep_refuses_a_fifth_chain():
    w = cases.lockstep_workload(16)
    stream = capi.new_stream()
    base = MCMC(w, seed=1, lut_output=False, consume=True, stream=stream)
    chains = [base] + [MCMC(w, seed=2 + c, lut_output=False, consume=True, stream=stream, share_with=base)
                       for c in range(cases.MAX_LOCKSTEP)]
    try:
        with pytest.raises(capi.SxmcError, match="2 to 4 chains"):
            nll.MultiGroup(chains)
        nll.MultiGroup(chains[:cases.MAX_LOCKSTEP]).close()
    finally:
        for m in chains[::-1]:
            close(m)


# ============================================================================================ (c) the one-workgroup end
# The cooperative step end is switched off in these walks: ONE launch behind the fill is then the one-workgroup form and
# nothing else, and two are the proof that it was not taken.
def tail_walks(case, end):
    w = case.workload()
    jw = widths_of(case, w)
    kw = dict(jump_width=jw, lut_output=case.lut_output, dense=case.dense)
    want, want_lut = reference(repr(case), w, **kw)
    for graph_steps in (0, GRAPH):
        m = new_chain(w, coop=False, tail=True, **kw)
        try:
            got, lut, ends = walk(m, graph_steps, lut_output=case.lut_output)
        finally:
            close(m)
        assert ends == {end}, (case, graph_steps, ends)
        all_same(got, want)
        if case.lut_output:
            assert np.array_equal(lut, want_lut), np.argwhere(lut != want_lut)[:4]
    return want_lut


@pytest.mark.parametrize("case", cases.TAIL_TAKEN + [cases.TAIL_WORDS_TAKEN], ids=repr)
def test_one_workgroup_end_at_its_limits(case):
    """256 and 255 look-ups as 16 x 16, 17 x 15, 1 x 256 and 256 x 1 (256 members and parameters: staged at exactly
    kStage); 65 536 histogram words."""
    assert case.one_workgroup
    tail_walks(case, ONE_LAUNCH)


@pytest.mark.parametrize("case", cases.TAIL_NOT_TAKEN + [cases.TAIL_WORDS_NOT_TAKEN], ids=repr)
def test_one_workgroup_end_is_not_taken_beyond_its_limits(case):
    """272 and 257 look-ups, 65 792 words: the two-launch form (the cooperative one being switched off)."""
    assert not case.one_workgroup
    tail_walks(case, TWO_LAUNCHES)


def test_one_workgroup_end_stores_the_lookup_table():
    """lut_output=True: rows are the events, every member stores its row of the table."""
    case = cases.TAIL_LUT
    lut = tail_walks(case, ONE_LAUNCH).view(np.float32).reshape(case.members, case.nevents)
    other = case.workload().events[:, -1] == 1.0
    assert np.all(lut[:, other] == 0) and np.all(np.isnan(lut[-1][~other])) and np.any(lut[0] > 0)


def test_one_workgroup_end_sums_256_rows_like_two_blocks():
    """1 x 256: the sequential event sum is two blocks of 128 rows, reduced by the finisher; one workgroup of 1024 lanes
    must round the same sums in the same order.  The NLL of EVERY step, not only of the two a flush shows, bit for bit."""
    case = cases.TAIL_TAKEN[2]
    assert (case.members, case.rows, case.blocks) == (1, 256, 2)
    w = case.workload()
    a = new_chain(w, coop=False, tail=True, rows=NSTEPS)
    b = new_chain(w, coop=False, tail=False, rows=NSTEPS)
    try:
        differ = []
        for k in range(NSTEPS):
            a.step()
            b.step()
            capi.synchronize()
            assert a.group.LastStepLaunches() - fills(a) == ONE_LAUNCH + (k == 0)
            assert b.group.LastStepLaunches() - fills(b) == TWO_LAUNCHES + (k == 0)
            if bits(a.proposed_nll.get())[0] != bits(b.proposed_nll.get())[0]:
                differ.append((k, a.proposed_nll.get()[0], b.proposed_nll.get()[0]))
        assert not differ, (len(differ), differ[:3])
        same(record(a), record(b))
    finally:
        close(a)
        close(b)


# ============================================================================================ (d) the fused step
@pytest.mark.parametrize("case", cases.FUSED, ids=repr)
def test_fused_step_at_sixteen_and_seventeen_members(case):
    """fill_step_kernel over the edge workload's ordered table: ONE launch per step."""
    w = case.workload()
    want, _ = reference(repr(case) + " ordered", w, ordering=True)
    for graph_steps in (0, GRAPH):
        m = new_chain(w, coop=True, fused=True, ordering=True)
        try:
            info = m.group.LaunchInfo()
            got, _, ends = walk(m, graph_steps)
        finally:
            close(m)
        assert "table=ordered" in info, info
        assert ends == {IN_THE_FILL}, (ends, info)
        all_same(got, want)


# ============================================================================================ (e) the host replay
def test_one_workgroup_end_follows_the_host_replay():
    case = cases.TAIL_TAKEN[0]
    w = case.workload()
    m = new_chain(w, coop=False, tail=True, rows=NSTEPS)
    try:
        r = Replay(m, w, SEED, NSTEPS)
        for k in range(NSTEPS):
            r.before()
            m.step()
            capi.synchronize()
            # (the fill + ONE launch; a chain's first step zeroes the histograms in a launch of its own before them)
            assert m.group.LastStepLaunches() - fills(m) == ONE_LAUNCH + (k == 0), k
            assert m.group.StepEndTimeouts() == 0
            r.after(r.vp, k % 8 == 0)
        assert 0 < r.accepted < NSTEPS, r.accepted
    finally:
        close(m)


def test_joint_lockstep_ends_follow_the_host_replay():
    members, classes = 17, [300, 40]
    w = cases.lockstep_workload(members)
    stream = capi.new_stream()
    base = MCMC(w, seed=1, lut_output=False, consume=True, stream=stream)
    chains, ls = [], None
    try:
        events = [cases.lockstep_events(members, k, c) for c, k in enumerate(classes)]
        for c in range(2):
            chains.append(new_chain(w, seed=SEED + c, stream=stream, share_with=base, data=events[c], rows=NSTEPS))
        ls = LockstepChains(chains)
        ls.mg.SetJointStepEnd(True)
        replays = [Replay(m, w, SEED + c, NSTEPS, events[c]) for c, m in enumerate(chains)]
        for k in range(NSTEPS):
            for r in replays:
                r.before()
            ls.step()
            capi.synchronize()
            for c, r in enumerate(replays):
                assert r.m.group.LastStepLaunches() - fills(r.m) == TWO_LAUNCHES + (k == 0), (k, c)
                r.after(r.vp, k % 8 == c)
        for r in replays:
            assert 0 < r.accepted < NSTEPS, r.accepted
    finally:
        if ls is not None:
            ls.close()
        for m in chains[::-1]:
            close(m)
        close(base)


def test_cooperative_lookahead_follows_the_host_replay():
    """Pass by pass, each allowed two steps.  One step: A was accepted.  Two: A was refused -- the replay refuses it from
    the oracle's NLL -- and B, the vector the shadow evaluators held, was decided from B's partial sums: its NLL is the
    oracle's at B."""
    case = cases.LOOKAHEAD[3]
    assert (case.members, case.classes, case.blocks) == (12, 129, 2)
    w = case.workload()
    rows = NSTEPS + 2
    m = new_chain(w, coop=True, rows=rows)
    la = LookaheadWalk(m, threads=0)
    try:
        la.bind(w.events)
        r = Replay(m, w, SEED, rows)
        twice = 0
        while r.ref.count < NSTEPS:
            r.before()
            vb = la.shadow.proposed_vector.get()
            la.cap.set(np.array([r.count + 2], np.int32))
            la.one_pass()
            capi.synchronize()
            assert m.group.LastStepLaunches() - fills(m) == ONE_LAUNCH + (r.k == 0), r.k
            assert m.group.StepEndTimeouts() == 0
            advanced = int(m.jump_counter.get()[0]) - r.count
            assert advanced in (1, 2), advanced
            if advanced == 1:
                r.after(r.vp, r.k % 8 == 0)
                assert int(m.accept_counter.get()[0]) == r.acc_before + 1       # (a pass stops at one step only if it accepts)
            else:
                twice += 1
                r.refused_unseen()
                r.proposal(vb)                                  # the look-ahead vector: the proposal after a rejection
                r.after(vb, True)
        assert 0 < r.accepted < r.ref.count and twice >= 1, (r.accepted, twice)
        assert la.passes < r.ref.count
    finally:
        la.close()
        close(m)
