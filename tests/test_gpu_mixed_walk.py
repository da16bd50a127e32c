"""GPU: sxmc::MCMC over a fit that mixes a histogram signal with two kernel-density signals (tests/cpp/mixed_walk.cpp),
walked in every form such a walk can take.  The MIXED form -- kernel members on the walk's stream, the histogram
members in their group, the event sum over both kinds of column, the whole step recordable -- must walk the
per-evaluator chain BIT FOR BIT: every recorded row, the NLL included, and the accepted count are compared as bytes
across the reference form, the defaults, lut_output, graph_steps = 16, consume = false and columns_in_place (the
histogram columns looked up inside the event sum; eager and recorded).  A kernel member no floating parameter touches is
evaluated at set-up only; one that reads floating parameters at every step.  A walk with the line's bandwidth scale at
1.01 must differ (the power check).  The same walks over a histogram of 40 x 40 x 40 bins
(beyond LDS: the group counts the event bins only) must agree in the same way."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NSTEPS = 3000


def run(*args):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "mixed.mk", "mixed_walk"])
    r = subprocess.run([os.path.join(CPP, "mixed_walk")] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_walks(out, events_about):
    walks = {w["setting"]: w for w in out["walks"]}
    assert list(walks) == ["reference_form", "defaults", "lut_output", "graph_steps_16", "no_consume", "bandwidth_1.01",
                           "in_place", "in_place_graph_16"]
    ref = walks["reference_form"]
    assert ref["form"] == "reference"
    assert ref["rows"] > 0 and ref["finite_nll_rows"] == ref["rows"] and 0 < ref["accepted"] < NSTEPS
    assert abs(ref["events"] - events_about) < 0.1 * events_about
    # the reference walk evaluates every evaluator at set-up and at every step
    assert ref["line_evaluations"] == NSTEPS + 1 and ref["pedestal_evaluations"] == NSTEPS + 1
    for name in ("defaults", "lut_output", "graph_steps_16", "no_consume", "in_place", "in_place_graph_16"):
        w = walks[name]
        assert w["form"] == "mixed", (name, w["form"])
        assert w["same_as_first"], name + ": the chain is not the per-evaluator chain bit for bit"
        assert w["hash"] == ref["hash"] and w["rows"] == ref["rows"] and w["accepted"] == ref["accepted"]
        assert w["pedestal_evaluations"] == 1, name       # no floating parameter touches it: the set-up evaluation alone
        if name.endswith("graph_steps_16") or name.endswith("graph_16"):
            # (a recorded launch counts once: set-up, the eager first run, 16 recorded steps, the runs' remainders)
            assert 1 + 16 < w["line_evaluations"] < NSTEPS + 1
        else:
            assert w["line_evaluations"] == NSTEPS + 1, name
    power = walks["bandwidth_1.01"]
    assert power["form"] == "mixed"
    assert not power["same_as_first"] and power["hash"] != ref["hash"]


def test_mixed_walk_is_the_per_evaluator_chain_bit_for_bit():
    check_walks(run(), 900)


def test_mixed_walk_over_a_histogram_beyond_lds():
    check_walks(run("--big"), 900)
