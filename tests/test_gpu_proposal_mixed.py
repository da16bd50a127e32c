"""The correlated proposal in the MIXED walk: tests/cpp/proposal_mixed_walk.cpp walks a fit of one histogram and two
kernel-density signals (two floating systematics, five parameters, 600 steps, burn-in 0.2) with
sxmc::Proposal::COVARIANCE.  The mixed form -- whose steps end in sxmc_group_finish_columns_step_async, or with
consume off in the plain step end through the group-less launch point -- walks its reference form's chain byte for byte,
also with lut_output, replayed from graphs of 16 steps, with columns_in_place, and asked with lookahead; that chain is
not the diagonal one, and its last factor is a dense triangle."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
MIXED = ["covariance, mixed", "covariance, lut_output", "covariance, graph_steps 16", "covariance, consume off",
         "covariance, columns_in_place", "covariance, columns_in_place, graph_steps 16", "covariance, lookahead"]


def field(line, name):
    words = line.split()
    return words[words.index(name) + 1]


@pytest.fixture(scope="module")
def walked():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "proposal.mk", "proposal_mixed_walk"])
    r = subprocess.run([os.path.join(CPP, "proposal_mixed_walk")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    return dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln)


def test_mixed_forms_walk_the_reference_form_chain(walked):
    want = walked["covariance, reference_form"]
    assert field(want, "form") == "reference" and field(want, "nrows") == "360" and field(want, "parameters") == "5"
    assert 0 < int(field(want, "accepted")) < 600
    assert field(want, "off_diagonal") == "10"                       # every parameter floats: a dense triangle
    for name in MIXED:
        got = walked[name]
        assert field(got, "form") == "mixed", (name, got)
        assert field(got, "fnv1a") == field(want, "fnv1a"), name
        assert field(got, "accepted") == field(want, "accepted"), name
        assert field(got, "off_diagonal") == "10", name


def test_the_chain_is_not_the_diagonal_one(walked):
    diagonal = walked["diagonal, reference_form"]
    assert field(diagonal, "off_diagonal") == "0"
    assert field(diagonal, "fnv1a") != field(walked["covariance, reference_form"], "fnv1a")
