"""The effective sample size of both proposal laws ON THE DEVICE, at the shape of tests/test_proposal_ess_cpu.py and
with its floor: tests/cpp/proposal_walk.cpp --ess walks four floated rates over one observable, of which two pairs look
alike (histograms of unit Gaussians at 3.0 / 3.15 and 7.0 / 7.15, 750 events of each, no systematic -- the walk does not
re-evaluate), 30 000 steps with burn-in 0.2, with sxmc::Proposal::DIAGONAL and ::COVARIANCE from the same seed, and
reports per law the pairs' correlations and ESS = rows / the largest autocorrelation time (Sokal's automatic window,
M >= 5 tau) over the rates.

Asserted, as on the host: the diagonal chain's |rho| of each look-alike pair is >= 0.9, and
ESS(covariance) >= 2 x ESS(diagonal).  (1 / (1 - rho^2) >= 5.3 at that rho for a Gaussian ridge; the floor is kept well
below it.  The histograms are filled from samples and the events are drawn from them, so the figures are not the
host replay's, whose PDFs are the exact bin integrals; the shape is.)"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def field(line, name):
    words = line.split()
    return words[words.index(name) + 1]


def test_covariance_doubles_the_effective_sample_size_on_the_device():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "proposal.mk", "proposal_walk"])
    r = subprocess.run([os.path.join(CPP, "proposal_walk"), "--ess"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    lines = dict(ln.split("\t", 1) for ln in r.stdout.splitlines() if "\t" in ln)
    diagonal, covariance = lines["ess diagonal"], lines["ess covariance"]
    assert field(diagonal, "steps") == field(covariance, "steps") == "30000"
    assert abs(float(field(diagonal, "rho01"))) >= 0.9 and abs(float(field(diagonal, "rho23"))) >= 0.9
    ratio = float(field(covariance, "ess")) / float(field(diagonal, "ess"))
    print("ESS ratio on the device: %.2f" % ratio)
    assert ratio >= 2.0
