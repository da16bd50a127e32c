"""Real event weights (sxmc_group_set_event_weights) through every sequential step end -- one-workgroup, cooperative,
two-launch, fused, sxmc_group_mcmc_step_async --, sxmc_group_eval_nll_async and the weighted launch point
(sxmc_launch_nll_event_chunks_weighted), on the shapes of tests/step_end_form_cases.py: 16 and 17 members; 1, 127, 128,
129 and 300 classes; the 256 look-ups of the one-workgroup end.  The law: tests/weighted_events_reference.py.

  1. weights of 1.0: partial sums, NLL and 50 steps of chain are the unweighted group's BYTES, in every form, with and
     without the lookup table, and through the launch point;
  2. integer weights in {1, 2, 3, 7} without the lookup table: the BYTES of the unweighted walk over the data set in which
     event i stands m_i times -- and not those of the unweighted walk over the events themselves;
  3. fractional weights in (0, 3), some exactly 0 in a class with a positive one: the NLL against the f64 reference to
     NLL_RTOL = 1e-12 (tests/test_gpu_nll.py's bound on the kernels: only the order of addition differs) -- classes,
     events, and the launch point at 1 x 64, 2 x 128 and 64 x 256 lanes over 1, 63, 64, 65 and 1000 events;
  4. refusals and state.

The walks: a first step in debug mode (it accepts: the chain's current NLL is then the step end's own sum, not the
launch point's of setup(), whose lanes cut the events otherwise), 49 steps eager, and again replayed from a graph of 16.
WHICH FORM RAN is asserted from the launches per step, as tests/test_gpu_step_end_forms.py does."""
import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, nll
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import MCMC, LockstepChains
from tests import step_end_form_cases as cases
from tests import weighted_events_reference as ref
from tests.test_gpu_nll import NLL_RTOL, oracle_nll_of_workload, random_nll_inputs
from tests.test_gpu_step_end_arith import bits, close, record, same
from tests.test_gpu_step_end_forms import IN_THE_FILL, ONE_LAUNCH, TWO_LAUNCHES, fills

pytestmark = pytest.mark.gpu

SEED = 5
NSTEPS, GRAPH = 50, 16

# form -> (switches, the step-end launches behind the fill)
FORMS = {
    "two-launch": (dict(coop=False, fused=False, tail=False), TWO_LAUNCHES),
    "cooperative": (dict(coop=True, fused=False, tail=True), ONE_LAUNCH),
    "one-workgroup": (dict(coop=False, fused=False, tail=True), ONE_LAUNCH),
    "fused": (dict(coop=True, fused=True, tail=True, ordering=True), IN_THE_FILL),
    "mcmc_step": (dict(coop=False, fused=False, tail=False), None),
}
# 16 / 17 members on each side of the member loop's sixteen; 127 / 128 / 129 rows on each side of a block of 128
COOPERATIVE = [cases.Case(16, 300), cases.Case(17, 300), cases.Case(16, 127), cases.Case(17, 128), cases.Case(16, 129)]
# 16 x 1 and 17 x 1 look-ups, and 16 x 16 = 256: the one-workgroup end's limit
ONE_WORKGROUP = [cases.Case(16, 1, nevents=400), cases.Case(17, 1, nevents=400), cases.TAIL_TAKEN[0]]
BEYOND_ONE_WORKGROUP = cases.TAIL_NOT_TAKEN[0]                # 16 x 17 look-ups
MCMC_STEP = [cases.Case(16, 300), cases.Case(17, 129)]
PLAN = ([("cooperative", c) for c in COOPERATIVE] + [("one-workgroup", c) for c in ONE_WORKGROUP] +
        [("fused", c) for c in cases.FUSED] + [("mcmc_step", c) for c in MCMC_STEP] +
        [("two-launch", cases.Case(17, 129))])
PLAN_IDS = ["%s-%r" % p for p in PLAN]


def chain(w, form, data=None, weights=None, lut_output=False):
    sw, _ = FORMS[form]
    step = form == "mcmc_step"
    m = MCMC(w, seed=SEED, lut_output=lut_output, consume=not step, fused="step" if step else True,
             stream=capi.new_stream())
    m.group.SetCooperativeStepEnd(sw["coop"])
    m.group.SetFusedStep(sw["fused"])
    m.group.SetTailKernel(sw["tail"])
    if sw.get("ordering"):
        m.group.SetOrdering(True, force=True)
    m.setup(w.events if data is None else data, sync_interval=NSTEPS, event_weights=weights)
    return m


def walk(m, graph_steps, form):
    m.step(debug_mode=True)
    m.steps(NSTEPS - 1, graph_steps)
    out = record(m)
    assert out["count"] == NSTEPS
    assert m.group.StepEndTimeouts() == 0
    want = FORMS[form][1]
    if want is not None:
        # the form is read off two more steps, launched behind the record: the first step after a replayed graph has a
        # zeroing launch in front of it, the second has none
        m.step()
        m.step()
        assert m.group.LastStepLaunches() - fills(m) == want, (form, m.group.LastStepLaunches(), fills(m))
    return out


_walked = {}


def walked(w, key, form, graph_steps=0, data=None, weights=None, lut_output=False):
    """One walk per key: computed once, shared, never modified."""
    key = (id(w), key, form, graph_steps, lut_output)
    if key not in _walked:
        m = chain(w, form, data, weights, lut_output)
        try:
            out = walk(m, graph_steps, form)
            out["lut"] = bits(m.lut.get()).copy() if lut_output else None
        finally:
            close(m)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _walked[key] = out
    return _walked[key]


def integer_weights(n, seed):
    return np.random.default_rng(seed).choice([1.0, 2.0, 3.0, 7.0], n)


def fractional_weights(w, seed):
    """Weights in (0, 3), a fifth of them exactly 0 -- and at least one zero in a class that also holds a positive one."""
    rng = np.random.default_rng(seed)
    n = w.events.shape[0]
    fw = rng.uniform(0.0, 3.0, n)
    fw[fw == 0.0] = 1.0
    fw[rng.uniform(size=n) < 0.2] = 0.0
    return fw


# ================================================================================================ 1. weights of 1.0
@pytest.mark.parametrize("form,case", PLAN, ids=PLAN_IDS)
def test_unit_weights_walk_the_unweighted_chain(form, case):
    w = case.workload()
    ones = np.ones(w.events.shape[0])
    want = walked(w, "unweighted", form)
    assert 1 < want["nacc"] < NSTEPS, want["nacc"]                     # both outcomes of a step occur
    for graph_steps in (0, GRAPH):
        same(walked(w, "ones", form, graph_steps, weights=ones), want)


def test_unit_weights_beyond_the_one_workgroup_limit():
    """16 x 17 look-ups with the cooperative end switched off: two launches, weighted or not."""
    case = BEYOND_ONE_WORKGROUP
    assert not case.one_workgroup
    w = case.workload()
    m = chain(w, "one-workgroup", weights=np.ones(w.events.shape[0]))
    try:
        m.step(debug_mode=True)
        m.steps(NSTEPS - 1)
        assert m.group.LastStepLaunches() - fills(m) == TWO_LAUNCHES
        got = record(m)
    finally:
        close(m)
    same(got, walked(w, "unweighted", "two-launch"))


@pytest.mark.parametrize("form,case", [("cooperative", cases.Case(16, 129)), ("one-workgroup", cases.TAIL_LUT),
                                       ("two-launch", cases.Case(17, 129)), ("mcmc_step", cases.Case(17, 129))],
                         ids=lambda x: x if isinstance(x, str) else repr(x))
def test_unit_weights_with_the_lookup_table(form, case):
    """Rows are the events: the weight array is indexed by event; the table is written as before."""
    w = case.workload()
    ones = np.ones(w.events.shape[0])
    want = walked(w, "unweighted", form, lut_output=True)
    got = walked(w, "ones", form, weights=ones, lut_output=True)
    same(got, want)
    assert np.array_equal(got["lut"], want["lut"])


@pytest.mark.parametrize("case", [cases.Case(16, 300), cases.Case(17, 129), cases.Case(16, 1, nevents=400)], ids=repr)
@pytest.mark.parametrize("lut_output", [False, True])
def test_unit_weights_give_the_partial_sums_of_eval_nll(case, lut_output):
    """sxmc_group_eval_nll_async: every partial sum, as bytes."""
    w = case.workload()
    sums = []
    for weights in (None, np.ones(w.events.shape[0])):
        m = chain(w, "two-launch", weights=weights, lut_output=lut_output)
        try:
            m.event_partial_sums.set(np.full(m.nnllthreads, 1e300))
            n = m.group.EvalNllAsync(m.stream, m.proposed_vector, m.nexpected, m.n_mc, m.source_id, m.normalizations,
                                     m.event_partial_sums)
            capi.synchronize()
            sums.append(bits(m.event_partial_sums.get()[:n]).copy())
        finally:
            close(m)
    assert sums[0].size == cases.sum_blocks(case.nevents if lut_output else case.classes)
    assert np.array_equal(sums[0], sums[1])


def launch_point(x, ne, ns, grid, block, weights):
    d = {k: DeviceArray(v) for k, v in x.items() if isinstance(v, np.ndarray)}
    sums = DeviceArray(np.full(grid * block, 1e300))
    if weights is None:
        nll.nll_event_chunks(grid, block, None, d["lut"], d["pars"], ne, ns, d["nexpected"], d["n_mc"], d["source_id"],
                             d["norms"], sums)
    else:
        nll.nll_event_chunks_weighted(grid, block, None, d["lut"], d["pars"], ne, ns, d["nexpected"], d["n_mc"],
                                      d["source_id"], d["norms"], sums, DeviceArray(weights))
    capi.synchronize()
    return sums.get()


LAUNCH_SHAPES = [(1, 64), (2, 128), (64, 256)]
LAUNCH_EVENTS = [1, 63, 64, 65, 1000]


@pytest.mark.parametrize("grid,block", LAUNCH_SHAPES)
@pytest.mark.parametrize("ne", LAUNCH_EVENTS)
def test_launch_point_with_unit_weights_is_the_unweighted_one(grid, block, ne):
    ns = 17
    x = random_nll_inputs(np.random.default_rng(ne + grid), ne, ns, 5)
    want = launch_point(x, ne, ns, grid, block, None)
    got = launch_point(x, ne, ns, grid, block, np.ones(ne))
    assert np.array_equal(bits(got), bits(want))


# ================================================================================================ 2. integer weights
@pytest.mark.parametrize("form,case", PLAN, ids=PLAN_IDS)
def test_integer_weights_walk_the_chain_of_the_repeated_events(form, case):
    w = case.workload()
    m = integer_weights(w.events.shape[0], 31 + case.members + case.classes)
    repeated = ref.repeat_events(w.events, m)
    assert repeated.shape[0] == int(m.sum()) > w.events.shape[0]
    want = walked(w, "repeated", "two-launch", data=repeated)
    for graph_steps in (0, GRAPH):
        same(walked(w, "integers", form, graph_steps, weights=m), want)
    # the control: the weights are not ignored
    plain = walked(w, "unweighted", form)
    assert not np.array_equal(plain["rows"], want["rows"])
    assert not np.array_equal(plain["current_nll"], want["current_nll"])


# ================================================================================================ 3. fractional weights
def reference_nll(w, v, weights):
    """The f64 NLL at v with the law's event term: the oracle's lookup table and nll_total, the reference's sum."""
    _, _, norms, lut = oracle_nll_of_workload(w, v)
    sig = w.signals
    ev = ref.weighted_event_sum(lut, v, [s.nexpected for s in sig], [s.n_mc for s in sig], [s.source_id for s in sig],
                                norms, weights)
    return oracle.nll_total(v, w.nsignals, w.nsources, w.parameter_means(), w.parameter_sigmas(), ev,
                            [s.nexpected for s in sig], [s.n_mc for s in sig], [s.source_id for s in sig], norms)


@pytest.mark.parametrize("form,case", [("cooperative", cases.Case(16, 300)), ("cooperative", cases.Case(17, 129)),
                                       ("one-workgroup", cases.TAIL_TAKEN[0]), ("two-launch", cases.Case(17, 128)),
                                       ("fused", cases.FUSED[1]), ("mcmc_step", cases.Case(16, 127))],
                         ids=lambda x: x if isinstance(x, str) else repr(x))
@pytest.mark.parametrize("lut_output", [False, True], ids=["classes", "events"])
def test_fractional_weights_against_the_f64_reference(form, case, lut_output):
    w = case.workload()
    fw = fractional_weights(w, 7 + case.members)
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    tables = np.stack([np.asarray(oracle.set_eval_points(geom, w.events, s.dataset)) for s in w.signals])
    _, class_of = ref.classes(tables)
    shared = [k for k in np.unique(class_of[fw == 0.0]) if np.any(fw[class_of == k] > 0)]
    assert shared or case.classes == 1                           # a zero weight in a class with a positive one
    m = chain(w, form, weights=fw, lut_output=lut_output)
    try:
        # setup()'s NLL at the means: the weighted launch point at the walk's 64 x 256 lanes
        want0 = reference_nll(w, w.parameter_means(), fw)
        got0 = m.current_nll.get()[0]
        print(form, case, "setup NLL", got0, want0, abs(got0 - want0) / abs(want0))
        v = m.proposed_vector.get()
        m.step(debug_mode=True)
        rows, nacc = m.flush()
        got = m.proposed_nll.get()[0]
        want = reference_nll(w, v, fw)
        plain = reference_nll(w, v, np.ones(fw.size))
        print(form, case, "step NLL", got, want, abs(got - want) / abs(want), "unweighted", plain)
        assert nacc == 1
        assert abs(got0 - want0) <= NLL_RTOL * abs(want0)
        assert abs(got - want) <= NLL_RTOL * abs(want)
        assert abs(plain - want) > 1e-3 * abs(want)              # the control: the weights matter at this scale
    finally:
        close(m)


@pytest.mark.parametrize("grid,block", LAUNCH_SHAPES)
@pytest.mark.parametrize("ne", LAUNCH_EVENTS)
def test_launch_point_with_fractional_weights(grid, block, ne):
    ns = 17
    rng = np.random.default_rng(100 + ne + grid)
    x = random_nll_inputs(rng, ne, ns, 5)
    fw = rng.uniform(0.0, 3.0, ne)
    fw[rng.uniform(size=ne) < 0.2] = 0.0
    got = launch_point(x, ne, ns, grid, block, fw)
    want = ref.chunk_sums(x["lut"], x["pars"], x["nexpected"], x["n_mc"], x["source_id"], x["norms"], fw, grid, block)
    lanes = min(ne, grid * block)
    assert np.all(got[lanes:] == 0.0)                            # lanes without events write their 0
    # per lane the same terms in the same order: what differs is the device's logarithm, to a few ulp of each term
    scale = np.maximum(np.abs(want), 1e-300)
    print("launch point", grid, block, ne, "worst lane", float(np.max(np.abs(got - want) / scale)))
    total, want_total = float(np.sum(got)), float(np.sum(want))
    assert abs(total - want_total) <= NLL_RTOL * max(abs(want_total), 1e-300)
    # the control: a weight read from the neighbouring event gives other sums
    assert ne == 1 or not np.allclose(got, ref.chunk_sums(x["lut"], x["pars"], x["nexpected"], x["n_mc"], x["source_id"],
                                                          x["norms"], np.roll(fw, 1), grid, block), rtol=1e-9, atol=0)


# ================================================================================================ 4. refusals and state
def test_a_weight_count_that_differs_from_the_points_is_refused_at_the_next_evaluation():
    case = cases.Case(16, 129)
    w = case.workload()
    for lut_output in (False, True):
        m = chain(w, "cooperative", lut_output=lut_output)
        try:
            m.group.SetEventWeights(np.ones(w.events.shape[0] - 1))          # (accepted: the count is the evaluation's matter)
            with pytest.raises(capi.SxmcError) as e:
                m.step()
            assert e.value.code == capi.ERR_STATE and "event weights" in str(e.value)
            with pytest.raises(capi.SxmcError) as e:
                m.group.EvalNllAsync(m.stream, m.proposed_vector, m.nexpected, m.n_mc, m.source_id, m.normalizations,
                                     m.event_partial_sums)
            assert e.value.code == capi.ERR_STATE
            m.group.SetEventWeights(None)
            m.step()
            capi.synchronize()
        finally:
            close(m)


@pytest.mark.parametrize("value,at", [(float("nan"), 3), (float("inf"), 0), (-1.0, 11), (-5e-324, 7)])
def test_weights_that_are_not_finite_and_non_negative_are_refused_by_index(value, at):
    case = cases.Case(16, 129)
    w = case.workload()
    m = chain(w, "cooperative")
    try:
        bad = np.ones(w.events.shape[0])
        bad[at] = value
        bad[-1] = -3.0
        with pytest.raises(capi.SxmcError) as e:
            m.group.SetEventWeights(bad)
        assert e.value.code == capi.ERR_INVALID
        assert ("event weight %d " % at) in str(e.value), str(e.value)
        assert ref.check_weights(bad)[0] == at
        m.step()                                                           # (the group is as it was: unweighted)
        capi.synchronize()
    finally:
        close(m)


def test_lockstep_lookahead_and_in_place_entries_refuse_a_weighted_group():
    case = cases.Case(16, 300)
    w = case.workload()
    ones = np.ones(w.events.shape[0])
    a = chain(w, "cooperative")
    b = MCMC(w, seed=SEED + 1, lut_output=False, consume=True, stream=a.stream, share_with=a)
    b.setup(w.events, sync_interval=NSTEPS)
    set_ = None
    try:
        assert a.group.LookaheadSupported()
        a.group.SetEventWeights(ones)
        assert not a.group.LookaheadSupported()
        set_ = LockstepChains([a, b])
        with pytest.raises(capi.SxmcError) as e:
            set_.step()
        assert e.value.code == capi.ERR_STATE and "event weights" in str(e.value)
        a.event_weights = DeviceArray(ones)                                # (as setup(event_weights=...) leaves it)
        with pytest.raises(ValueError, match="event weights"):
            set_.step()
        a.event_weights = None
        # the look-ahead entry, asked directly
        with pytest.raises(capi.SxmcError) as e:
            set_.mg.LookaheadStepAsync(a.stream, a.proposed_vector, a.normalizations)
        assert e.value.code == capi.ERR_STATE and "event weights" in str(e.value)
        # look-ups in place
        a.group.SetColumns(list(range(w.nsignals)))
        sums = DeviceArray.zeros(64 * 256, np.float64)
        with pytest.raises(capi.SxmcError) as e:
            a.group.EvalColumnsNllAsync(a.stream, None, w.events.shape[0], a.proposed_vector, a.nexpected, a.n_mc,
                                        a.source_id, a.normalizations, sums)
        assert e.value.code == capi.ERR_STATE and "event weights" in str(e.value)
        a.group.SetEventWeights(None)
        assert a.group.LookaheadSupported()
    finally:
        if set_ is not None:
            set_.close()
        close(b)
        close(a)


def test_weights_set_cleared_and_set_again_on_one_group():
    """One group, one data set: unweighted, integer weights, unweighted again, other weights -- each evaluation's partial
    sums are those of a fresh group in that state."""
    case = cases.Case(17, 129)
    w = case.workload()
    n = w.events.shape[0]
    states = [None, integer_weights(n, 1), None, fractional_weights(w, 2), integer_weights(n, 1)]

    def sums_of(m):
        m.event_partial_sums.set(np.full(m.nnllthreads, 1e300))
        k = m.group.EvalNllAsync(m.stream, m.proposed_vector, m.nexpected, m.n_mc, m.source_id, m.normalizations,
                                 m.event_partial_sums)
        capi.synchronize()
        return bits(m.event_partial_sums.get()[:k]).copy()

    fresh = []
    for weights in states[:4]:
        m = chain(w, "two-launch", weights=weights)
        try:
            fresh.append(sums_of(m))
        finally:
            close(m)
    fresh.append(fresh[1])
    assert not np.array_equal(fresh[0], fresh[1]) and not np.array_equal(fresh[1], fresh[3])
    m = chain(w, "two-launch")
    try:
        for weights, want in zip(states, fresh):
            m.group.SetEventWeights(weights)
            assert np.array_equal(sums_of(m), want)
    finally:
        close(m)


def test_weights_cannot_be_set_while_recording_and_a_graph_of_16_steps_equals_eager():
    case = cases.Case(16, 300)
    w = case.workload()
    fw = fractional_weights(w, 3)
    eager = walked(w, "fractional", "cooperative", 0, weights=fw)
    same(walked(w, "fractional", "cooperative", GRAPH, weights=fw), eager)
    m = chain(w, "cooperative", weights=fw)
    try:
        m.step()
        with capi.Graph.capture(m.stream) as g:
            m._recording = True
            try:
                m.step()
                with pytest.raises(capi.SxmcError) as e:
                    m.group.SetEventWeights(np.ones(fw.size))
                assert e.value.code == capi.ERR_STATE and "recording" in str(e.value)
            finally:
                m._recording = False
        g.close()
    finally:
        close(m)


# ================================================================================================ the reference form
def reference_form_chain(w, weights):
    """mcmc.MCMC(fused=False): group.EvalAsync, then the event sum over the whole table through the launch point."""
    m = MCMC(w, seed=SEED, fused=False, lut_output=True, consume=False, stream=capi.new_stream())
    m.setup(w.events, sync_interval=NSTEPS, event_weights=weights)
    return m


def test_the_python_reference_form_sums_through_the_weighted_launch_point():
    """Unit weights: the unweighted chain's bytes.  Fractional weights: the step's NLL against the f64 reference."""
    case = cases.Case(17, 129)
    w = case.workload()
    records = []
    for weights in (None, np.ones(w.events.shape[0])):
        m = reference_form_chain(w, weights)
        try:
            m.step(debug_mode=True)
            m.steps(NSTEPS - 1)
            records.append(record(m))
        finally:
            close(m)
    assert 1 < records[0]["nacc"] < NSTEPS
    same(records[1], records[0])
    fw = fractional_weights(w, 5)
    m = reference_form_chain(w, fw)
    try:
        v = m.proposed_vector.get()
        m.step(debug_mode=True)
        m.flush()
        got, want = m.proposed_nll.get()[0], reference_nll(w, v, fw)
        print("reference form", got, want, abs(got - want) / abs(want))
        assert abs(got - want) <= NLL_RTOL * abs(want)
        assert abs(reference_nll(w, v, np.ones(fw.size)) - want) > 1e-3 * abs(want)
    finally:
        close(m)
