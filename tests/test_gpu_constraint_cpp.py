"""Correlated constraints in the C++ walker: tests/cpp/constraint_walk.cpp walks the small fit (tests/cpp/small_fit.h: 3
signals, a shift and a resolution systematic floating, 600 steps, burn-in 0.2) with MCMC::constraint_correlation in every
sequential form and writes the fit and its chain out; the Python walker then walks the SAME fit.

  * under each law -- no matrix, rho = I, rho(shift, resolution) = -0.6 -- every form (consuming, replayed from graphs of
    16 steps, asked with lookahead, batched, the reference's launches, with the lookup table) walks one chain, byte for
    byte, and none of them took the look-ahead pass; so with the covariance proposal, weighted events and a weighted
    histogram member;
  * rho = I is the chain of no matrix, as bytes, everywhere; the correlated chain is another one;
  * the mixed histogram + kernel-density fit (constraint_walk --mixed): the reference's launches, the MIXED form, its
    graphs, columns_in_place (the columns step end) and asked with lookahead, the same three laws;
  * mcmc.MCMC.walk(constraint_correlation=...) over the dumped fit, started from the C++ walk's initial widths
    (tests/test_gpu_proposal_cpp.py, cpp_widths, says why), gives the C++ chain's bytes and the C++ whitening matrix's;
  * a chain of a lockstep set, a matrix that is not positive definite, a correlated parameter without a constraint and a
    matrix of the wrong size are refused by name, and the chain walks on afterwards."""
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi
from sxmc_amd.mcmc import MCMC
from tests.test_gpu_proposal_cpp import cpp_widths, field, small_fit_workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LAWS = ("none", "identity", "correlated")
FORMS = ["consuming", "graph_steps 16", "lookahead", "lookahead, graph_steps 16", "consume off", "reference_form",
         "lut_output"]
FEW = FORMS[:3]
MIXED = ["reference_form", "mixed", "graph_steps 16", "columns_in_place", "columns_in_place, graph_steps 16", "lookahead"]


def run(args, timeout=300):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "constraints.mk", "constraint_walk"])
    r = subprocess.run([os.path.join(CPP, "constraint_walk")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    return dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln)


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    out = tmp_path_factory.mktemp("constraint_walk")
    return run([str(out)]), str(out)


@pytest.fixture(scope="module")
def mixed():
    return run(["--mixed"])


def one_chain(lines, prefix, forms, nrows, matrix):
    first = lines[prefix + forms[0]]
    assert field(first, "nrows") == str(nrows)
    for f in forms:
        line = lines[prefix + f]
        assert field(line, "fnv1a") == field(first, "fnv1a"), prefix + f
        assert field(line, "accepted") == field(first, "accepted"), prefix + f
        if matrix:
            assert field(line, "passes") == "0", prefix + f              # no look-ahead pass was launched
        assert field(line, "whitening") == str(matrix) and line.split()[-1] == first.split()[-1], prefix + f
    return field(first, "fnv1a"), field(first, "accepted")


@pytest.mark.parametrize("setting,forms", [("", FORMS), ("covariance, ", FEW), ("weighted events, ", FEW),
                                           ("sample weights, ", FEW)])
def test_every_sequential_form_walks_one_chain_under_each_law(walked, setting, forms):
    lines, _ = walked
    chains = {law: one_chain(lines, law + ", " + setting, forms, 360, 0 if law == "none" else 25) for law in LAWS}
    assert chains["identity"] == chains["none"]
    assert chains["correlated"][0] != chains["none"][0]
    assert 0 < int(chains["correlated"][1]) < 600
    if not setting:
        assert field(lines["correlated, lookahead"], "form") == "consuming"
        assert field(lines["correlated, lookahead, graph_steps 16"], "form") == "consuming"
        assert field(lines["correlated, consume off"], "form") == "batched"
        assert field(lines["correlated, reference_form"], "form") == "reference"
        # with a matrix the walk asked with lookahead never takes the pass; without one this fit would
        assert field(lines["none, lookahead"], "form") in ("lookahead", "consuming")


def test_the_mixed_walk_and_its_columns_step_end(mixed):
    chains = {law: one_chain(mixed, law + ", ", MIXED, 180, 0 if law == "none" else 25) for law in LAWS}
    assert chains["identity"] == chains["none"]
    assert chains["correlated"][0] != chains["none"][0]
    assert field(mixed["correlated, mixed"], "form") == "mixed"
    assert field(mixed["correlated, columns_in_place"], "form") == "mixed"
    assert field(mixed["correlated, reference_form"], "form") == "reference"


def test_refusals_name_their_reason(walked):
    lines, _ = walked
    assert "lockstep set has no step end with correlated constraints" in lines["correlated, in a lockstep set"]
    assert "not positive definite at parameter 4" in lines["not positive definite"]
    assert "parameter 0 has no constraint" in lines["unconstrained"]
    assert "16 entries for 5 x 5" in lines["wrong size"]
    assert lines["after the refusals"].split() == ["nrows", "12"]


@pytest.mark.parametrize("law,graph_steps", [("correlated", 0), ("correlated", 16), ("none", 16)])
def test_python_walker_gives_the_cpp_chain_as_bytes(walked, law, graph_steps):
    lines, out = walked
    w = small_fit_workload(out)
    P = w.nparameters
    assert P == 5
    want = np.fromfile(os.path.join(out, "chain.f32" if law == "correlated" else "chain_none.f32"),
                       np.float32).reshape(-1, P + 1)
    want_W = np.fromfile(os.path.join(out, "whitening.f64"), np.float64)
    assert want.shape[0] == 360 and want_W.size == P * P
    widths = cpp_widths(out, w)
    rho = None
    if law == "correlated":
        rho = np.eye(P)
        rho[3, 4] = rho[4, 3] = -0.6
    m = MCMC(w, seed=7, lut_output=False, consume=True, stream=capi.new_stream())
    m.initial_jump_widths = lambda fixed=None: widths.copy()
    try:
        chain, accepted = m.walk(w.events, 600, 0.2, sync_interval=150, graph_steps=graph_steps,
                                 constraint_correlation=rho)
        W = m.ConstraintWhitening()
    finally:
        capi.synchronize()
        if m._graph is not None:
            m._graph.close()
        for p in m.pdfs:
            p.close()
        m.group.close()
    assert accepted == int(field(lines[law + ", consuming"], "accepted"))
    assert chain.tobytes() == want.tobytes(), np.argwhere(chain.view(np.uint32) != want.view(np.uint32))[:4]
    if law == "none":
        assert W is None
        return
    assert np.ascontiguousarray(W.T).tobytes() == want_W.tobytes()
    assert W[4, 3] == 0.75 and W[4, 4] == 1.25 and np.count_nonzero(W - np.diag(np.diag(W))) == 1
