"""The cases of the step-end replay tests, shared by tests/test_step_reference_cpu.py (which runs the host reference
alone over every case and asserts the conditions the seeds were chosen for) and tests/test_gpu_step_replay.py (which
follows the device through the same cases).  TEST INFRASTRUCTURE ONLY.

(a) synthetic tables in the style of random_nll_inputs (tests/test_gpu_nll.py): NaN and 0 look-ups, fewer sources than
    parameters, one constrained rate;
(b) small workloads with awkward events and a signal of norm 0, walked with both re-tunings.
"""
import functools
import math

import numpy as np

from oracle import oracle
from tests.step_reference import StepReference, replay_walk

NSTEPS = 200                 # (a): steps per case
WALK_STEPS, WALK_BURNIN = 120, 0.2          # (b): re-tunings at steps 24 and 48, 72 rows kept
MIN_REJECTIONS = MIN_UPHILL_ACCEPTED = 20   # an ordinary case decides both ways often enough ...
MIN_MARGIN = 1e-4            # ... and never so closely that the 1e-12 allowed on an NLL could move a decision


class Case:
    def __init__(self, name, nsources, nsyst, ns, ne, seed, width, fixed=(), count0=0, accepted0=0, offset0=0,
                 kind="ordinary"):
        self.name, self.nsources, self.nsyst, self.ns, self.ne = name, nsources, nsyst, ns, ne
        self.P = nsources + nsyst
        self.seed, self.width, self.kind = seed, width, kind
        self.fixed = tuple(range(self.P)) if fixed == "all" else tuple(fixed)
        self.count0, self.accepted0, self.offset0 = count0, accepted0, offset0

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def tables(self):
        """lut, means, sigmas, nexpected, n_mc, norms, source_id, the start vector and the jump widths."""
        rng = np.random.default_rng(1000 + self.P * 7 + self.ns)
        ne, ns, nsources, nsyst = self.ne, self.ns, self.nsources, self.nsyst
        lut = rng.uniform(0.0, 2.0, size=(ns, ne)).astype(np.float32)
        lut[rng.uniform(size=lut.shape) < 0.05] = np.nan          # empty-histogram look-ups
        lut[rng.uniform(size=lut.shape) < 0.05] = 0.0
        start = np.concatenate([rng.uniform(0.5, 1.5, nsources), rng.normal(0, 0.1, nsyst)])
        means = np.concatenate([np.ones(nsources), np.zeros(nsyst)])
        sigmas = np.concatenate([np.zeros(nsources), np.full(nsyst, 0.1)])
        sigmas[0] = 0.3
        nexpected = rng.uniform(10, 100, ns)
        n_mc = rng.integers(1000, 100000, ns).astype(np.uint32)
        norms = (n_mc * rng.uniform(0.3, 1.0, ns)).astype(np.uint32)
        source_id = (np.arange(ns) % nsources).astype(np.int16)
        nexpected *= ne / float(np.sum(nexpected * norms / n_mc))   # rates of 1 expect the ne events there are
        # widths: `width` x the scale each parameter moves the NLL by one unit over, / sqrt(free parameters)
        nfree = max(1, self.P - len(self.fixed))
        per_source = np.zeros(nsources)
        for j in range(ns):
            per_source[source_id[j]] += nexpected[j] * norms[j] / n_mc[j]
        unit = np.concatenate([1.0 / np.sqrt(per_source), np.full(nsyst, 0.1)])
        jw = (self.width * unit / math.sqrt(nfree)).astype(np.float32)
        if self.kind == "negative rates":
            # a source mean near 0 and a wide jump: the chain starts among negative rates (NLL 1e18, every proposal that
            # stays there is accepted: exp(0) = 1 >= u), comes out once, and is then refused every way back
            means[0], start[0], jw[0] = 0.02, -2.0, 0.5
        if self.kind == "infinite":
            # ONE event, every look-up 0 or NaN (the event sum is 0).  +inf comes from the last parameter's constraint,
            # whose square overflows beyond |p| = 1.34e-6: the chain starts there, proposals that stay there give
            # inf - inf (rejected), one that lands inside is finite (accepted)
            lut = np.where(rng.uniform(size=(ns, 1)) < 0.5, np.float32(0.0), np.float32(np.nan)).astype(np.float32)
            sigmas[-1], means[-1], start[-1], jw[-1] = 1e-160, 0.0, 2e-6, 2e-6
        jw[list(self.fixed)] = -1.0
        if self.kind == "ordinary":
            # the start: where a short chain of numpy's own generator has taken the vector, so that the replayed steps
            # are those of a chain in equilibrium (uphill and downhill proposals, both accepted and refused)
            def nll_at(v):
                return oracle.full_nll(lut, v, ne, ns, nsources, means, sigmas, nexpected, n_mc, source_id, norms)[0]
            cur, free = nll_at(start), jw > 0
            for _ in range(1500):
                v = np.where(free, start + jw.astype(np.float64) * rng.normal(size=self.P), start)
                new = nll_at(v)
                if new < cur or rng.uniform() <= math.exp(cur - new):
                    start, cur = v, new
        return dict(lut=np.ascontiguousarray(lut), means=means, sigmas=sigmas, nexpected=nexpected, n_mc=n_mc,
                    norms=norms, source_id=source_id, start=start, jump_width=jw)

    def oracle_nll(self, vector):
        t = self.tables()
        return oracle.full_nll(t["lut"], vector, self.ne, self.ns, self.nsources, t["means"], t["sigmas"],
                               t["nexpected"], t["n_mc"], t["source_id"], t["norms"])[0]

    def offsets0(self):
        return [self.offset0 + 3 * i for i in range(self.P)] if self.offset0 else [0] * self.P

    def new_reference(self, fill=0.0):
        t = self.tables()
        return StepReference(self.seed, t["jump_width"], t["start"], self.oracle_nll(t["start"]),
                             self.count0 + NSTEPS + 1, offsets=self.offsets0(), accepted=self.accepted0,
                             count=self.count0, fill=fill)

    def replay_alone(self):
        """The reference over its own proposals, every NLL from the oracle."""
        ref = self.new_reference()
        ref.first_proposal()
        for _ in range(NSTEPS):
            ref.step(self.oracle_nll(ref.v_proposed))
        return ref


def check_conditions(case, ref):
    """The conditions a case's seed was chosen for, on the reference's record of a whole chain."""
    s = ref.summary()
    d = ref.decisions
    assert s["steps"] == NSTEPS
    if case.kind == "uniform is 1":
        # generator 0's word 0 is 0xFFFFFFFF at step 100: u = 1.0 = exp(0) on a tie, which `<=` accepts and `<` would
        # not.  All parameters are fixed, so from step 1 on the device's two NLLs are one number: an exact tie there too.
        assert d[ONE_AT_STEP]["u"] == 1.0 and d[ONE_AT_STEP]["margin"] == 0.0 and d[ONE_AT_STEP]["accept"]
        assert min(r["margin"] for k, r in enumerate(d) if k != ONE_AT_STEP) >= MIN_MARGIN, (case, s)
        assert s["accepted"] == NSTEPS and all(r["nll_proposed"] == r["nll_current"] for r in d), (case, s)
        return s
    assert s["min_margin"] >= MIN_MARGIN, (case, s)
    if case.kind == "ordinary":
        assert s["rejections"] >= MIN_REJECTIONS and s["uphill_accepted"] >= MIN_UPHILL_ACCEPTED, (case, s)
    elif case.kind == "all fixed":
        # the proposal IS the current vector: every step a tie, exp(0) = 1 >= u
        assert s["accepted"] == NSTEPS and all(r["nll_proposed"] == r["nll_current"] for r in d), (case, s)
    elif case.kind == "negative rates":
        ties = sum(r["accept"] and r["nll_current"] == 1e18 and r["nll_proposed"] == 1e18 for r in d)
        out = sum(r["accept"] and r["nll_current"] == 1e18 and r["nll_proposed"] < 1e17 for r in d)
        back = sum((not r["accept"]) and r["nll_proposed"] == 1e18 for r in d)
        assert ties >= 5 and out == 1 and back >= 20, (case, ties, out, back)
    elif case.kind == "infinite":
        inf = math.inf
        assert d[0]["nll_current"] == inf
        both = sum((not r["accept"]) and r["nll_current"] == inf and r["nll_proposed"] == inf for r in d)
        out = sum(r["accept"] and r["nll_current"] == inf and r["nll_proposed"] < inf for r in d)
        back = sum((not r["accept"]) and r["nll_current"] < inf and r["nll_proposed"] == inf for r in d)
        assert both >= 1 and out == 1 and back >= 5, (case, both, out, back)
    else:
        raise AssertionError(case.kind)
    return s


# Philox4x32-10 with key (1, 0) and counter (offset, generator 0) gives word 0 = 0xFFFFFFFF at this offset (found by
# search; test_step_reference_cpu.py checks it): the one uniform in 2^32 that is exactly 1
ONE_AT_OFFSET, ONE_AT_STEP = 1711450034, 100

# P on each side of the 256 the one-workgroup step end stages (kStage), the signals on each side of it with few
# parameters, and of the event sum's 16-signal request groups; seeds and widths: see test_step_reference_cpu.py
CASES = [
    Case("P1", 1, 0, 1, 37, seed=1, width=2.0),
    Case("P2", 1, 1, 1, 37, seed=1, width=0.7),
    Case("P31", 5, 26, 7, 100, seed=1, width=1.2),
    Case("P256", 12, 244, 12, 100, seed=1, width=2.0),
    Case("P257", 12, 245, 12, 100, seed=1, width=1.2),
    Case("P300", 29, 271, 29, 100, seed=1, width=1.2),
    Case("ns1", 1, 5, 1, 64, seed=1, width=1.2),
    Case("ns16", 4, 2, 16, 64, seed=1, width=0.7),
    Case("ns17", 4, 2, 17, 64, seed=1, width=2.0),
    Case("ns256", 3, 2, 256, 20, seed=1, width=1.2),
    Case("ns257", 3, 2, 257, 20, seed=1, width=0.7),
    Case("P300_ns257", 29, 271, 257, 20, seed=1, width=1.2),
    Case("parameter0_fixed", 4, 2, 6, 64, seed=1, width=2.0, fixed=(0,)),
    Case("all_fixed", 4, 2, 6, 64, seed=1, width=1.2, fixed="all", kind="all fixed"),
    Case("uniform_is_1", 4, 2, 6, 64, seed=1, width=1.2, fixed="all", offset0=ONE_AT_OFFSET - ONE_AT_STEP,
         kind="uniform is 1"),
    Case("counters_above_0", 4, 2, 6, 64, seed=1, width=0.7, count0=7, accepted0=3, offset0=2 ** 32 - 90),
    Case("negative_rates", 3, 2, 5, 64, seed=1, width=1.2, kind="negative rates"),
    Case("infinite", 2, 2, 3, 1, seed=1, width=1.2, fixed=(0, 1, 2), kind="infinite"),
]
CASE = {c.name: c for c in CASES}
# the one-workgroup step end at other workgroup sizes than the walk's 128: over the cases whose loops depend on it
BLOCK_CASES = ["P1", "P31", "P257", "P300", "ns257", "parameter0_fixed"]
BLOCKS = [64, 96, 1024]


# ---------------------------------------------------------------------------------------------- (b) walks
def _oracle_nll_of_workload():
    from tests.test_gpu_nll import oracle_nll_of_workload       # (the module imports without a GPU)
    return oracle_nll_of_workload


def walk_workload(name):
    """config 3 at 1/500 with 2000 events, or config 1 -- with events the look-up must not trip over (outside the
    domain, in bins no signal fills, of a second data set, forty in one bin) and one more signal whose samples all lie
    outside the domain (norm 0).  "c3/N": the first N events of the config 3 workload."""
    from sxmc_amd import workloads
    if name == "c1":
        w = workloads.config1()
        w.events[:40] = w.events[0]
        w.events[40:45, :w.nobs] = 1e9                     # outside the domain
        w.events[45:60, -1] = 1.0                          # a data set no signal belongs to
        far = np.tile(np.array([[50.0, 50.0, 0.0]], np.float32), (500, 1))         # energy beyond [5, 15)
        w.signals.append(workloads.Signal(far, 3, nexpected=30.0, source_id=2))
        return w
    w = workloads.config3(0.002, nevents=2000)
    ev = w.events
    ev[1:40] = ev[1]                                       # many events in one bin
    ev[40:45, :w.nobs] = 1e9                               # outside the domain
    ev[45:50, :w.nobs] = np.array([9.97, 0.02, -0.99], np.float32)   # a corner bin no sample reaches
    ev[50:300:2, -1] = 1.0                                 # events of the second data set ...
    w.signals[3].dataset = 1                               # ... which two signals belong to
    w.signals[7].dataset = 1
    far = workloads.config3_signal_table(np.random.default_rng(77), 0, 700)
    far[:, 0] += 50.0                                      # energy and true energy beyond [0, 10): no sample is counted
    far[:, 3] += 50.0
    w.signals.append(workloads.Signal(far, 5, nexpected=40.0, source_id=12))
    if "/" in name:
        w.events = np.ascontiguousarray(ev[: int(name.split("/")[1])])
    return w


# workload -> the seeds walked over it (the first: every form; all of them: the lockstep set)
WALKS = {"c3": (1, 2), "c1": (1, 2), "c3/1": (1, 2), "c3/255": (1, 2), "c3/257": (1, 2)}


@functools.lru_cache(maxsize=None)
def workload_cached(name):
    return walk_workload(name)


@functools.lru_cache(maxsize=None)
def replayed_walk(name, seed):
    """The host replay of MCMC.walk(w.events, WALK_STEPS, WALK_BURNIN) from `seed`: every NLL from
    oracle_nll_of_workload at the replay's own vector.  Computed once, shared, never modified."""
    from sxmc_amd.mcmc import MCMC
    w = workload_cached(name)
    nll_of = _oracle_nll_of_workload()
    jw = MCMC.initial_jump_widths(_Widths(w))
    rows, accepted, ref, steps = replay_walk(lambda v: nll_of(w, v)[0], seed, w.parameter_means(), jw, WALK_STEPS,
                                             WALK_BURNIN)
    rows.setflags(write=False)
    return rows, accepted, ref, steps


class _Widths:
    """What MCMC.initial_jump_widths reads of a chain (mcmc.cpp:198-228 on the host: no device needed)."""

    def __init__(self, w):
        self.w, self.nparameters, self.nsignals = w, w.nparameters, w.nsignals


def check_walk_conditions(name, seed, ref):
    s = ref.summary()
    assert s["steps"] == WALK_STEPS
    assert s["min_margin"] >= MIN_MARGIN, (name, seed, s)
    assert s["rejections"] >= MIN_REJECTIONS and s["uphill_accepted"] >= MIN_UPHILL_ACCEPTED, (name, seed, s)
    return s


if __name__ == "__main__":       # the figures the seeds were chosen by: python -m tests.step_replay_cases
    for c in CASES:
        print(c.name, c.seed, c.replay_alone().summary())
    for name, seeds in WALKS.items():
        for seed in seeds:
            print(name, seed, replayed_walk(name, seed)[2].summary())
