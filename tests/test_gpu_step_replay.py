"""The END of an MCMC step on the device -- the uniform, `np < nc || u <= exp(nc - np)`, the jump-buffer row, the next
proposal -- against a host replay that shares no code with it (tests/step_reference.py: Philox words from
tests/helpers.py, NLL values from the CPU oracle).  The other chain tests run in debug mode (every step accepted) or
compare the walking forms with each other, and every form ends its steps in one device function: a wrong word of the
generator's output, a swapped order of draws, the proposed vector in the row of a rejected step or a proposal centred on
the rejected vector would pass all of them.

(a) the launch points, step by step, 200 steps without debug mode per case: the reference's separate launches
    (nll_event_chunks, nll_event_reduce, nll_total, jump_decider, pick_new_vector) and finish_nll_jump_pick_combo;
(b) the walking forms, free-running over small workloads with both re-tunings.

The cases, their seeds and the conditions they were chosen for (asserted on the reference alone, also without a GPU:
tests/test_step_reference_cpu.py) are in tests/step_replay_cases.py.
"""
import numpy as np
import pytest

from sxmc_amd import capi, nll
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import MCMC, LockstepChains
from tests import step_replay_cases as cases
from tests.test_gpu_nll import NLL_RTOL

pytestmark = pytest.mark.gpu

FILL = -7.5                  # what the jump buffer's rows hold before a step writes them


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def nll_close(got, want):
    return got == want or abs(got - want) <= NLL_RTOL * abs(want)


class Chain:
    """One case's buffers on the device, as mcmc.cpp:159-256 sets them up."""

    def __init__(self, case):
        t = case.tables()
        P = case.P
        self.case, self.t = case, t
        self.d = {k: DeviceArray(t[k]) for k in ("lut", "means", "sigmas", "nexpected", "n_mc", "norms", "source_id")}
        self.jw = DeviceArray(t["jump_width"])
        self.rngs = nll.make_rngs(P, case.seed)
        capi.synchronize()
        if case.offset0:
            st = self.rngs.get().reshape(P, 4)
            st[:, 2] = case.offsets0()
            self.rngs.set(st.ravel())
        self.v_cur, self.v_prop = DeviceArray(t["start"].copy()), DeviceArray(np.full(P, np.nan))
        self.nll_cur = DeviceArray(np.array([case.oracle_nll(t["start"])]))
        self.nll_prop = DeviceArray.zeros(1, np.float64)
        self.acc, self.cnt = DeviceArray(np.array([case.accepted0], np.int32)), DeviceArray(np.array([case.count0], np.int32))
        self.nrows = case.count0 + cases.NSTEPS + 1
        self.jb = DeviceArray(np.full(self.nrows * (P + 1), FILL, np.float32))
        self.total = DeviceArray.zeros(1, np.float64)

    def offsets(self):
        st = self.rngs.get().reshape(self.case.P, 4)
        assert np.all(st[:, 0] == self.case.seed) and np.array_equal(st[:, 1], np.arange(self.case.P, dtype=np.uint64))
        return [int(o) for o in st[:, 2]]


def follow(case, launch_step, pick_grid=1):
    """The device through NSTEPS steps of `case`, the reference beside it.  launch_step(chain): one step's launches."""
    c = Chain(case)
    t, P = c.t, case.P
    ref = case.new_reference(fill=FILL)
    nll.pick_new_vector(pick_grid, 64, None, P, c.rngs, c.jw, c.v_cur, c.v_prop)        # mcmc.cpp:252-256
    ref.first_proposal()
    capi.synchronize()
    assert c.offsets() == ref.offsets
    jw = np.clip(t["jump_width"].astype(np.float64), 0.0, None)
    free = t["jump_width"] > 0
    v_cur, nll_cur, jb = c.v_cur.get(), c.nll_cur.get()[0], c.jb.get().reshape(c.nrows, P + 1)
    assert np.array_equal(bits(v_cur), bits(t["start"])) and np.all(jb == FILL)
    acc_before = case.accepted0
    for k in range(cases.NSTEPS):
        # the proposal: cur + jw * z.  1e-12 is the project's bound on a device normal (test_gpu_nll.py,
        # test_philox_known_answers_and_stream_layout), |z| < 6.7 as u1 >= 2^-32, and the addition rounds once
        vp = c.v_prop.get()
        tol = 8e-12 * jw + 2.0 ** -52 * np.abs(ref.v_proposed)
        err = np.abs(vp - ref.v_proposed)
        assert np.all(err <= tol), (k, int(np.argmax(err - tol)), vp, ref.v_proposed)
        assert np.array_equal(bits(vp[~free]), bits(v_cur[~free])), k       # fixed parameters: the current value itself
        want = case.oracle_nll(vp)
        count = ref.count
        launch_step(c)
        capi.synchronize()
        rec = ref.step(want, v_proposed=vp)
        got = c.nll_prop.get()[0]
        assert nll_close(got, want), (k, got, want)
        acc, cnt = int(c.acc.get()[0]), int(c.cnt.get()[0])
        assert acc - acc_before in (0, 1), (k, acc, acc_before)
        accepted, acc_before = acc - acc_before == 1, acc
        assert accepted == rec["accept"], (k, rec, got)
        # the state the decision implies, bit for bit
        v_cur = vp if accepted else v_cur
        nll_cur = got if accepted else nll_cur
        assert np.array_equal(bits(c.v_cur.get()), bits(v_cur)), k
        assert bits(c.nll_cur.get())[0] == bits(np.array([nll_cur]))[0], (k, c.nll_cur.get()[0], nll_cur)
        # row `count` of the jump buffer: their float casts; every other row untouched
        with np.errstate(over="ignore"):
            jb[count, :P] = v_cur.astype(np.float32)
            jb[count, P] = np.float32(nll_cur)
        got_jb = c.jb.get().reshape(c.nrows, P + 1)
        assert np.array_equal(bits(got_jb), bits(jb)), (k, count, np.argwhere(bits(got_jb) != bits(jb))[:4])
        assert np.array_equal(bits(got_jb[:, :P]), bits(ref.jump_buffer[:, :P])), k
        assert acc == ref.accepted and cnt == ref.count == count + 1, (k, acc, cnt)
        assert c.offsets() == ref.offsets, k
    s = cases.check_conditions(case, ref)          # (the chain followed IS the chain the seed was chosen on)
    alone = case.replay_alone().summary()
    assert (s["accepted"], s["rejections"], s["uphill_accepted"]) == (alone["accepted"], alone["rejections"],
                                                                      alone["uphill_accepted"])
    return ref


SHAPES = [(1, 64, 64), (2, 64, 128), (3, 96, 96), (2, 128, 1024)]      # event sum: grid, block; reduction: lanes


def shape_of(case):
    return SHAPES[cases.CASES.index(case) % len(SHAPES)]


def event_chunks(c, grid, block):
    case, d = c.case, c.d
    if not hasattr(c, "sums"):
        c.sums = DeviceArray.zeros(grid * block, np.float64)
    nll.nll_event_chunks(grid, block, None, d["lut"], c.v_prop, case.ne, case.ns, d["nexpected"], d["n_mc"],
                         d["source_id"], d["norms"], c.sums)


@pytest.mark.parametrize("case,pick_grid", [(c, 1) for c in cases.CASES] + [(cases.CASE["P300"], 3)],
                         ids=lambda v: repr(v))
def test_separate_launches_step_by_step(case, pick_grid):
    """mcmc.cpp's unfused sequence: MCMC::nll at the proposal (three launches), jump_decider, pick_new_vector -- the
    latter also as a grid of 3 x 64 lanes, which 300 parameters need two rounds of."""
    grid, block, red = shape_of(case)

    def step(c):
        d = c.d
        event_chunks(c, grid, block)
        nll.nll_event_reduce(1, red, None, grid * block, c.sums, c.total)
        nll.nll_total(1, 1, None, case.P, c.v_prop, case.ns, case.nsources, d["means"], d["sigmas"], c.total,
                      d["nexpected"], d["n_mc"], d["source_id"], d["norms"], c.nll_prop)
        nll.jump_decider(1, 1, None, c.rngs, c.nll_cur, c.nll_prop, c.v_cur, c.v_prop, case.P, c.acc, c.cnt, c.jb)
        nll.pick_new_vector(pick_grid, 64, None, case.P, c.rngs, c.jw, c.v_cur, c.v_prop)

    follow(case, step, pick_grid)


@pytest.mark.parametrize("case,block", [(c, 128) for c in cases.CASES] +
                         [(cases.CASE[n], b) for b in cases.BLOCKS for n in cases.BLOCK_CASES], ids=lambda v: repr(v))
def test_finish_combo_step_by_step(case, block):
    """finish_nll_jump_pick_combo, the one-workgroup step end every walking form ends in: staged (at most 256
    parameters and signals) and not, in workgroups of one wave, one and a half, two (the walk's) and sixteen."""
    grid, eblock, _ = shape_of(case)

    def step(c):
        d = c.d
        event_chunks(c, grid, eblock)
        nll.finish_nll_jump_pick_combo(1, block, None, grid * eblock, c.sums, case.ns, case.nsources, d["means"],
                                       d["sigmas"], c.rngs, c.nll_cur, c.nll_prop, c.v_cur, c.v_prop, c.acc, c.cnt,
                                       c.jb, case.P, c.jw, d["nexpected"], d["n_mc"], d["source_id"], d["norms"], False)

    follow(case, step)


# ---------------------------------------------------------------------------------------------- (b) the walking forms
def close(m):
    capi.synchronize()
    if m._graph is not None:
        m._graph.close()
    for p in m.pdfs:
        p.close()
    m.group.close()


def walk_in_form(w, form, seed):
    """MCMC.walk in one form -> [(chain, accepted, seed)]."""
    n, b = cases.WALK_STEPS, cases.WALK_BURNIN
    if form in ("reference", "fused", "step"):
        m = MCMC(w, seed=seed, fused={"reference": False, "fused": True, "step": "step"}[form])
        out = m.walk(w.events, n, b, sync_interval=50)
    else:
        lut_output = form in ("consume", "consume, no tail")
        m = MCMC(w, seed=seed, lut_output=lut_output, consume=True, stream=capi.new_stream())
        m.tail = form != "consume, no tail"
        out = m.walk(w.events, n, b, sync_interval=50, graph_steps=7 if form == "graph" else 0,
                     lookahead=form == "lookahead")
        if w.events.shape[0] >= 2000:        # (the small problems walk sequentially whatever is asked: see walk())
            assert form != "lookahead" or 0 < m.lookahead_passes < n
            assert form != "graph" or m._graph is not None
    close(m)
    return out


def check_walk(name, seed, chain, accepted):
    """A device walk against the host replay of the same seed (every NLL of the replay: the oracle at the replay's own
    vector): the same steps accepted and repeated, parameters to the float store plus the drift of the additions so
    far, the NLL column to the project's bound for a float-stored NLL (1e-6, test_gpu_nll.py)."""
    rows, ref_accepted, ref, steps = cases.replayed_walk(name, seed)
    cases.check_walk_conditions(name, seed, ref)
    assert accepted == ref_accepted and chain.shape == rows.shape, (accepted, ref_accepted, chain.shape, rows.shape)
    repeated = np.all(bits(chain[1:]) == bits(chain[:-1]), axis=1)
    want_repeated = np.array([not ref.decisions[i]["accept"] for i in steps[1:]])
    assert np.array_equal(repeated, want_repeated), np.flatnonzero(repeated != want_repeated)
    P = rows.shape[1] - 1
    jw = np.clip(np.max(np.array(ref.width_history, np.float64), axis=0), 0.0, None)   # each parameter's widest width
    ref64, got64 = rows.astype(np.float64), chain.astype(np.float64)
    tol = 2.0 ** -24 * np.abs(ref64[:, :P]) + (steps[:, None] + 1) * 8e-12 * jw
    err = np.abs(got64[:, :P] - ref64[:, :P])
    assert np.all(err <= tol), (np.argwhere(err > tol)[:4], err.max())
    assert np.all(np.abs(got64[:, P] - ref64[:, P]) <= 1e-6 * np.abs(ref64[:, P]))


FORMS = ["reference", "fused", "step", "consume", "consume, no tail", "classes", "graph", "lookahead"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(cases.WALKS))
def test_walking_forms_against_the_host_replay(name, form):
    w = cases.workload_cached(name)
    seed = cases.WALKS[name][0]
    chain, accepted = walk_in_form(w, form, seed)
    check_walk(name, seed, chain, accepted)


@pytest.mark.parametrize("name", list(cases.WALKS))
def test_lockstep_chains_against_the_host_replay(name):
    """Two chains of different seeds advanced together (one fill pass per step for both): each is ITS seed's replay."""
    w = cases.workload_cached(name)
    seeds = cases.WALKS[name]
    stream = capi.new_stream()
    base = MCMC(w, seed=seeds[0], lut_output=False, consume=True, stream=stream)
    chains = [base] + [MCMC(w, seed=s, lut_output=False, consume=True, stream=stream, share_with=base)
                       for s in seeds[1:]]
    for m in chains:
        m.walk_begin(w.events, cases.WALK_STEPS, cases.WALK_BURNIN, sync_interval=50)
    ls = LockstepChains(chains)
    i = 0
    for f in chains[0].flush_schedule():
        for m in chains:
            m._retune_if_due(i)
        ls.steps(f - i + 1)
        for m in chains:
            m._flush_if_due(f)
        i = f + 1
    for m, seed in zip(chains, seeds):
        chain, accepted = m.walk_end()
        check_walk(name, seed, chain, accepted)
    ls.close()
    for m in chains[::-1]:
        close(m)
