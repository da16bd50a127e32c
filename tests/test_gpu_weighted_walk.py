"""Weighted data events through whole walks of both walkers: tests/cpp/weighted_walk.cpp walks the small fit
(tests/cpp/small_fit.h: 3 signals, a shift and a resolution systematic floating, 600 steps, burn-in 0.2 -- both
re-tunings fall inside) with integer weights in {1, 2, 3, 7} and, beside it, the data set in which event i stands m_i
times; then the Python walker walks the SAME fit with the same weights.

  * in every sequential form -- the defaults (consuming), replayed from graphs of 16 steps, the reference's launches
    (the weighted launch point), batched, asked with lookahead -- with the diagonal and with the covariance proposal, the
    weighted walk's chain is the chain over the repeated events, byte for byte, and not the unweighted walk's;
  * asked with lookahead, a weighted walk goes sequentially (the walk over the repeated events beside it takes the pass);
  * mcmc.MCMC.walk(event_weights=...) over the dumped fit, from the C++ walk's initial widths
    (tests/test_gpu_proposal_cpp.py, cpp_widths, says why), gives the C++ chain's bytes, eager and replayed;
  * a chain of a lockstep set, columns_in_place, a count that is not the data's and a negative weight are refused by name.
"""
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi
from sxmc_amd.mcmc import MCMC
from tests.test_gpu_proposal_cpp import cpp_widths, small_fit_workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
FORMS = {"defaults": "consuming", "graph_steps 16": "consuming", "reference_form": "reference", "consume off": "batched",
         "lookahead asked": "consuming", "covariance": "consuming", "covariance, graph_steps 16": "consuming",
         "covariance, reference_form": "reference"}


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    out = tmp_path_factory.mktemp("weighted_walk")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "weighted.mk", "weighted_walk"])
    r = subprocess.run([os.path.join(CPP, "weighted_walk"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    return dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln), str(out)


def parts(line):
    """{"unweighted" | "weighted" | "repeated": {field: value}} of one case's line."""
    words = line.split()
    out = {}
    for which in ("unweighted", "weighted", "repeated"):
        i = words.index(which)
        out[which] = dict(zip(words[i + 1:i + 9:2], words[i + 2:i + 10:2]))
    return out


@pytest.mark.parametrize("name", sorted(FORMS))
def test_integer_weights_walk_the_chain_of_the_repeated_events(walked, name):
    lines, _ = walked
    p = parts(lines[name])
    assert p["weighted"]["nrows"] == "360" and 0 < int(p["weighted"]["accepted"]) < 600
    assert p["weighted"]["form"] == FORMS[name], p
    assert p["weighted"]["fnv1a"] == p["repeated"]["fnv1a"], p
    assert p["weighted"]["accepted"] == p["repeated"]["accepted"], p
    assert p["weighted"]["fnv1a"] != p["unweighted"]["fnv1a"], p           # the control: the weights are not ignored


def test_the_forms_walk_one_weighted_chain_and_lookahead_goes_sequentially(walked):
    lines, _ = walked
    first = parts(lines["defaults"])["weighted"]["fnv1a"]
    for name in ("graph_steps 16", "consume off", "lookahead asked"):
        assert parts(lines[name])["weighted"]["fnv1a"] == first, name
    cov = parts(lines["covariance"])["weighted"]["fnv1a"]
    assert cov != first and parts(lines["covariance, graph_steps 16"])["weighted"]["fnv1a"] == cov
    assert parts(lines["lookahead asked"])["repeated"]["form"] in ("lookahead", "consuming")


def test_refusals_name_their_reason(walked):
    lines, _ = walked
    assert "lockstep set has no weighted step end" in lines["refusal: in a lockstep set"]
    assert "columns_in_place has no weighted event sum" in lines["refusal: columns_in_place"]
    assert "449 event weights for 450 events" in lines["refusal: a count that is not the data's"]
    assert "event weight 5 " in lines["refusal: a negative weight"]


@pytest.mark.parametrize("graph_steps", [0, 16])
def test_python_walker_gives_the_cpp_chain_as_bytes(walked, graph_steps):
    lines, out = walked
    w = small_fit_workload(out)
    P = w.nparameters
    want = np.fromfile(os.path.join(out, "chain.f32"), np.float32).reshape(-1, P + 1)
    weights = np.fromfile(os.path.join(out, "weights.f64"), np.float64)
    assert want.shape[0] == 360 and weights.size == w.events.shape[0] == 450
    assert set(np.unique(weights)) == {1.0, 2.0, 3.0, 7.0}
    widths = cpp_widths(out, w)
    m = MCMC(w, seed=7, lut_output=False, consume=True, stream=capi.new_stream())
    m.initial_jump_widths = lambda fixed=None: widths.copy()
    try:
        chain, accepted = m.walk(w.events, 600, 0.2, sync_interval=150, graph_steps=graph_steps, event_weights=weights)
    finally:
        capi.synchronize()
        if m._graph is not None:
            m._graph.close()
        for p in m.pdfs:
            p.close()
        m.group.close()
    assert accepted == int(parts(lines["defaults"])["weighted"]["accepted"])
    assert chain.tobytes() == want.tobytes(), np.argwhere(chain.view(np.uint32) != want.view(np.uint32))[:4]


# ---------------------------------------------------------------------------------- a fit with kernel-density columns
MIXED_FORMS = {"mixed": "mixed", "mixed, graph_steps 16": "mixed", "mixed, consume off": "mixed", "mixed, lut_output": "mixed",
               "mixed, covariance": "mixed", "mixed, reference_form": "reference"}


@pytest.fixture(scope="module")
def mixed_walked():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "weighted.mk", "weighted_walk"])
    r = subprocess.run([os.path.join(CPP, "weighted_walk"), "--mixed"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    return dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln)


@pytest.mark.parametrize("name", sorted(MIXED_FORMS))
def test_mixed_fit_integer_weights_walk_the_chain_of_the_repeated_events(mixed_walked, name):
    """The MIXED form (kernel-density columns evaluated on the walk's stream, the weighted launch point over the whole
    table, the columns step end) and the reference form over the same fit."""
    p = parts(mixed_walked[name])
    assert p["weighted"]["nrows"] == "360" and 0 < int(p["weighted"]["accepted"]) < 600
    assert p["weighted"]["form"] == MIXED_FORMS[name], p
    assert p["weighted"]["fnv1a"] == p["repeated"]["fnv1a"], p
    assert p["weighted"]["accepted"] == p["repeated"]["accepted"], p
    assert p["weighted"]["fnv1a"] != p["unweighted"]["fnv1a"], p


def test_mixed_forms_walk_one_weighted_chain_and_in_place_is_refused(mixed_walked):
    first = parts(mixed_walked["mixed"])["weighted"]["fnv1a"]
    for name in ("mixed, graph_steps 16", "mixed, consume off", "mixed, lut_output", "mixed, reference_form"):
        assert parts(mixed_walked[name])["weighted"]["fnv1a"] == first, name
    assert "columns_in_place has no weighted event sum" in mixed_walked["refusal: mixed, columns_in_place"]
