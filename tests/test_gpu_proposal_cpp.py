"""The correlated proposal in the C++ walker: tests/cpp/proposal_walk.cpp walks the small fit (tests/cpp/small_fit.h:
3 signals, a shift and a resolution systematic floating, 600 steps, burn-in 0.2) with sxmc::Proposal::COVARIANCE in every
sequential form and writes the fit and its chain out; the Python walker then walks the SAME fit.

  * every form -- consuming, replayed from graphs of 16 steps, asked with lookahead, batched, the reference's launches,
    with the lookup table -- walks one chain, byte for byte, and none of them took the look-ahead pass;
  * that chain is not the diagonal one, the shrinkage matters, and at shrinkage 1 (T = I) it IS the diagonal chain;
  * mcmc.MCMC.walk(proposal="covariance") over the dumped fit, started from the C++ walk's initial widths (cpp_widths
    says why), gives the C++ chain's bytes and the C++ factor's bytes (both walkers re-tune through
    sxmc_proposal_factor; the Python walk is held to the host replay step by step in tests/test_gpu_proposal_walk.py),
    and so does the diagonal walk, the control;
  * a chain of a lockstep set refuses the proposal, naming the reason.
"""
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, workloads
from sxmc_amd.mcmc import MCMC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SEQUENTIAL = ["covariance", "covariance, graph_steps 16", "covariance, lookahead",
              "covariance, lookahead, graph_steps 16", "covariance, consume off", "covariance, reference_form",
              "covariance, lut_output"]


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    out = tmp_path_factory.mktemp("proposal_walk")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "proposal.mk", "proposal_walk"])
    r = subprocess.run([os.path.join(CPP, "proposal_walk"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln)
    print(r.stdout)
    return lines, str(out)


def field(line, name):
    words = line.split()
    return words[words.index(name) + 1]


def test_every_sequential_form_walks_one_chain(walked):
    lines, _ = walked
    first = lines["covariance"]
    assert field(first, "nrows") == "360" and 0 < int(field(first, "accepted")) < 600
    for name in SEQUENTIAL:
        assert field(lines[name], "fnv1a") == field(first, "fnv1a"), name
        assert field(lines[name], "accepted") == field(first, "accepted"), name
        assert field(lines[name], "factor") == "25" and lines[name].split()[-1] == first.split()[-1], name
        assert float(field(lines[name], "shrinkage")) == 0.05
        assert field(lines[name], "passes") == "0", name           # no look-ahead pass was launched
    assert field(lines["covariance, lookahead"], "form") == "consuming"
    assert field(lines["covariance, lookahead, graph_steps 16"], "form") == "consuming"
    assert field(lines["covariance, consume off"], "form") == "batched"
    assert field(lines["covariance, reference_form"], "form") == "reference"


def test_the_chain_is_not_the_diagonal_one_and_the_shrinkage_matters(walked):
    lines, _ = walked
    hashes = {name: field(lines[name], "fnv1a") for name in ("diagonal", "covariance", "covariance, shrinkage 0.5")}
    assert len(set(hashes.values())) == 3, hashes
    # at shrinkage 1 nothing of the correlations is left: T = I, L = diag(w), and fma(w, z, 0) is w * z rounded once --
    # the diagonal proposal's own bits, through the correlated code path
    assert field(lines["covariance, shrinkage 1"], "fnv1a") == hashes["diagonal"]
    assert field(lines["covariance, shrinkage 1"], "accepted") == field(lines["diagonal"], "accepted")
    assert field(lines["diagonal"], "factor") == "0"
    assert float(field(lines["covariance, shrinkage 0.5"], "shrinkage")) == 0.5
    assert float(field(lines["covariance, shrinkage 1"], "shrinkage")) == 1.0


def test_a_chain_of_a_lockstep_set_refuses_it(walked):
    lines, _ = walked
    said = lines["covariance, in a lockstep set"]
    assert "lockstep set has no correlated step end" in said, said


def small_fit_workload(out):
    """tests/cpp/small_fit.h from the tables and events the C++ program wrote."""
    signals = []
    for j in range(3):
        tab = np.fromfile(os.path.join(out, "table%d.f32" % j), np.float32).reshape(-1, 4)
        assert tab.shape[0] == 20000 + 777 * j
        signals.append(workloads.Signal(tab, 4, nexpected=100.0 + 50.0 * j, source_id=j))
    events = np.fromfile(os.path.join(out, "data.f32"), np.float32).reshape(-1, 3)
    systs = [dict(type="shift", obs=1, pars=[0]), dict(type="resolution_scale", obs=0, true_obs=2, pars=[1])]
    return workloads.Workload("small_fit", 2, [0.0, 0.0], [1.0, 2.0], [12, 9], signals, systs, [0.05, 0.1], events,
                              "tests/cpp/small_fit.h")


def cpp_widths(out, w):
    """The widths the C++ walk started from.  THE TWO LAYERS' INITIAL WIDTHS DIFFER IN THE LAST FLOAT BIT, with either
    proposal and since before this one: mcmc.h evaluates mcmc.cpp's `0.1 * width * scale_factor` in double and rounds to
    float once, as the reference does; mcmc.MCMC.initial_jump_widths multiplies numpy float32 scalars, which from numpy
    2 on stay float32 and round after each product.  Chains that start from widths an ulp apart drift apart in their
    last float bits.  What this file compares is the proposal's law in the two walkers, so the Python walker is handed
    the C++ walker's widths; the diagonal walk is compared the same way beside it, as the control."""
    widths = np.fromfile(os.path.join(out, "widths.f32"), np.float32)
    own = MCMC.initial_jump_widths(_Widths(w))
    assert widths.shape == own.shape and np.allclose(widths, own, rtol=2.0 ** -22, atol=0)     # an ulp or two, no more
    return widths


class _Widths:
    def __init__(self, w):
        self.w, self.nparameters, self.nsignals = w, w.nparameters, w.nsignals


@pytest.mark.parametrize("proposal,graph_steps", [("covariance", 0), ("covariance", 16), ("diagonal", 16)])
def test_python_walker_gives_the_cpp_chain_as_bytes(walked, proposal, graph_steps):
    lines, out = walked
    w = small_fit_workload(out)
    P = w.nparameters
    assert P == 5
    name = "chain.f32" if proposal == "covariance" else "chain_diagonal.f32"
    want = np.fromfile(os.path.join(out, name), np.float32).reshape(-1, P + 1)
    want_factor = np.fromfile(os.path.join(out, "factor.f64"), np.float64)
    assert want.shape[0] == 360 and want_factor.size == P * P
    widths = cpp_widths(out, w)
    m = MCMC(w, seed=7, lut_output=False, consume=True, stream=capi.new_stream())
    m.initial_jump_widths = lambda fixed=None: widths.copy()
    try:
        chain, accepted = m.walk(w.events, 600, 0.2, sync_interval=150, graph_steps=graph_steps, proposal=proposal)
        L, used = m.ProposalFactor()
    finally:
        capi.synchronize()
        if m._graph is not None:
            m._graph.close()
        for p in m.pdfs:
            p.close()
        m.group.close()
    assert accepted == int(field(lines[proposal], "accepted"))
    assert chain.tobytes() == want.tobytes(), np.argwhere(chain.view(np.uint32) != want.view(np.uint32))[:4]
    if proposal == "diagonal":
        assert L is None
        return
    assert used == 0.05 and np.ascontiguousarray(L.T).tobytes() == want_factor.tobytes()
    assert np.count_nonzero(np.tril(L, -1)) == P * (P - 1) // 2          # every parameter floats: a dense triangle
