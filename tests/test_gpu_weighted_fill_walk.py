"""GPU: walks over weighted Monte Carlo samples (sample multiplicities, include/sxmc_hip.h) as BYTES.  With every
m = 8 and n_mc = 8 n the chain is the unweighted walk's (bins, norm and n_mc all carry the scale: it cancels exactly);
with m in 0 ... 3 it is the walk over the tables with row i repeated m_i times.  3 signals of a few thousand rows, shift +
resolution scale, 300 steps through both re-tunings, in every sequential form of the Python walker; the C++ walker
(sxmc::MCMC, its MIXED form beside a kernel-density signal included) is tests/cpp/sample_weights_walk.cpp below."""
import functools
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, ensemble, mcmc, workloads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS, BURNIN = 300, 0.2       # re-tunings after steps 60 and 120
SYSTS = [dict(type="shift", obs=1, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=2, pars=[1])]
SIGMAS = [0.05, 0.05]
ROWS = (3001, 2500, 1999)


@functools.lru_cache(maxsize=None)
def tables():
    rng = np.random.default_rng(77)
    out = []
    for j, n in enumerate(ROWS):
        e_true = rng.normal(3.0 + j, 1.5, size=n)
        e = e_true + rng.normal(0.0, 0.4, size=n)
        r = 6.0 * rng.uniform(0.0, 1.0, size=n) ** (1.0 / 3.0)
        t = np.stack([e, r, e_true, np.zeros(n)], axis=1).astype(np.float32)
        t.setflags(write=False)
        out.append(t)
    mult = [rng.integers(0, 4, size=n).astype(np.uint32) for n in ROWS]
    return out, mult


@functools.lru_cache(maxsize=None)
def events(nevents):
    rng = np.random.default_rng(78)
    tabs, _ = tables()
    rows = np.concatenate([t[rng.integers(0, len(t), size=nevents // 3), :2] for t in tabs])
    ev = np.zeros((rows.shape[0], 3), np.float32)
    ev[:, :2] = rows
    return ev


def workload(kind, nevents):
    """"plain": the tables as they are; "times8": every multiplicity 8; "mult": m in 0 ... 3; "repeated": row i m_i times."""
    tabs, mult = tables()
    signals = []
    for j, (t, m) in enumerate(zip(tabs, mult)):
        table = np.repeat(t, m.astype(np.int64), axis=0) if kind == "repeated" else t
        s = workloads.Signal(table, 4, nexpected=60.0 + 20 * j, source_id=j)
        if kind == "times8":
            s.multiplicities = np.full(len(t), 8, np.uint32)
        if kind == "mult":
            s.multiplicities = m
        signals.append(s)
    return workloads.Workload("weighted-" + kind, 2, [0.0, 0.0], [10.0, 6.0], [20, 12], signals, SYSTS, SIGMAS,
                              events(nevents), "3 signals, shift + resolution scale")


# form -> (MCMC keywords, walk keywords, events, settings on the group)
FORMS = {
    "consuming": (dict(fused=True, lut_output=False, consume=True), {}, 900, {}),
    "two_launch": (dict(fused=True, lut_output=False, consume=True), {}, 900, dict(coop=False)),
    "one_workgroup": (dict(fused=True, lut_output=False, consume=True), {}, 45, {}),
    "reference_form": (dict(fused=False), {}, 900, {}),
    "batched": (dict(fused=True), {}, 900, {}),
    "graphs_of_16": (dict(fused=True, lut_output=False, consume=True), dict(graph_steps=16), 900, {}),
    "asked_with_lookahead": (dict(fused=True, lut_output=False, consume=True), dict(lookahead=True), 900, {}),
    "drop_in": (dict(fused="dropin"), {}, 900, {}),
}


def walk(kind, form):
    kw, walk_kw, nevents, settings = FORMS[form]
    w = workload(kind, nevents)
    stream = None if kw.get("fused") == "dropin" else capi.new_stream()
    m = mcmc.MCMC(w, seed=4242, stream=stream, **kw)
    if settings.get("coop") is False:
        m.group.SetCooperativeStepEnd(False)
    chain, accepted = m.walk(w.events, NSTEPS, BURNIN, sync_interval=100, **walk_kw)
    info = m.group.LaunchInfo()
    passes, launches = m.lookahead_passes, m.group.LastStepLaunches() if kw.get("consume") else None
    n_mc = m.n_mc.get().tolist()
    for p in m.pdfs:
        p.close()
    m.group.close()
    return dict(chain=np.ascontiguousarray(chain), accepted=accepted, info=info, passes=passes, launches=launches, n_mc=n_mc)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_walks_as_bytes(form):
    tabs, mult = tables()
    plain, times8 = walk("plain", form), walk("times8", form)
    assert times8["n_mc"] == [8 * n for n in ROWS] and "weighted" in times8["info"] and "weighted" not in plain["info"]
    assert 0 < plain["accepted"] < NSTEPS
    assert times8["accepted"] == plain["accepted"] and times8["chain"].tobytes() == plain["chain"].tobytes()
    weighted, repeated = walk("mult", form), walk("repeated", form)
    assert weighted["n_mc"] == [int(m.sum()) for m in mult] == repeated["n_mc"]
    assert weighted["accepted"] == repeated["accepted"] and weighted["chain"].tobytes() == repeated["chain"].tobytes()
    assert weighted["chain"].tobytes() != plain["chain"].tobytes()      # (the weights matter)
    if form == "asked_with_lookahead":
        print("look-ahead passes: plain %d, times8 %d, weighted %d" % (plain["passes"], times8["passes"], weighted["passes"]))
        assert times8["passes"] == 0 and weighted["passes"] == 0      # weighted: sequentially, whatever the plain walk took
    if form == "one_workgroup":
        assert weighted["launches"] == plain["launches"]               # the same step end after the fill's launch
    if form in ("consuming", "two_launch"):
        assert weighted["launches"] == repeated["launches"]


def test_lockstep_refuses_by_name():
    w = workload("mult", 900)
    stream = capi.new_stream()
    chains = [mcmc.MCMC(w, seed=1 + k, stream=stream, fused=True, lut_output=False, consume=True) for k in range(2)]
    for c in chains:
        c.setup(w.events, sync_interval=16)
    st = mcmc.LockstepChains(chains)
    with pytest.raises(ValueError, match="sample multiplicities"):
        st.step()
    with pytest.raises(capi.SxmcError, match="sample multiplicities set: lockstep sets") as err:
        st.mg.StepAsync(stream)                                          # the library's own refusal
    assert err.value.code == capi.ERR_STATE
    with pytest.raises(ValueError, match="sample multiplicities"):
        ensemble.run_experiments_in_lockstep(w, [1, 2], 10, [st])
    assert chains[0].group.LookaheadSupported() is False
    for c in chains:
        for p in c.pdfs:
            p.close()
        c.group.close()


def test_cpp_walker_as_bytes():
    """sxmc::MCMC over the same kinds of signal, every sequential form, the MIXED form beside a kernel-density signal:
    the program compares the chains itself and prints one line per form."""
    exe = os.path.join(ROOT, "tests", "cpp", "sample_weights_walk")
    assert os.access(exe, os.X_OK), exe + " is missing: __graft_entry__.build() makes it (tests/cpp/sampleweights.mk)"
    said = ""
    for args in ([], ["two_launch"]):     # (the two-launch step end is a setting of the whole process)
        done = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        print(done.stdout)
        assert done.returncode == 0, done.stdout + done.stderr
        said += done.stdout
    for form in ("consuming", "two_launch", "one_workgroup", "reference_form", "consume_off", "graphs_of_16", "mixed",
                 "lookahead_asked", "lockstep_refused"):
        assert ("ok " + form + "\t") in said, said
    assert "forms mixed mixed" in [l for l in said.splitlines() if l.startswith("ok mixed")][0], said
