"""CPU: what correlated constraints are for, fixed without a GPU.  Two parameters the likelihood does not depend on, each
with a Gaussian constraint, walk in the host replay (tests/step_reference.py; the NLL is the constraints' alone, by the
law of tests/step_reference_constraints.py): with rho = 0.9 between them the kept rows' sample correlation must lie
within 5 standard errors of 0.9, and with no matrix within 5 standard errors of 0.

The standard error of a sample correlation from n_eff independent draws of a bivariate Gaussian is
(1 - rho^2) / sqrt(n_eff); n_eff = n / tau with tau the larger integrated autocorrelation time of the two columns, by
Sokal's automatic window as in tests/test_proposal_ess_cpu.py.  tests/test_gpu_constraint_posterior.py walks the same
chain on the device."""
import math

import numpy as np

from tests import step_reference_constraints as sc
from tests.step_reference import replay_walk
from tests.test_proposal_ess_cpu import tau_sokal

NSTEPS, BURNIN, SEED = 30000, 0.2, 3
MEANS, SIGMAS, RHO = np.array([1.0, -2.0]), np.array([0.5, 0.02]), 0.9


def initial_widths():
    """mcmc.cpp:198-228 for two constrained parameters: 0.1 * sigma * (float)(2.4^2 / 2)."""
    return (0.1 * SIGMAS.astype(np.float32) * np.float32(2.4 * 2.4 / 2)).astype(np.float32)


def nll_of(W):
    return lambda v: sc.nll_total(0.0, v, MEANS, SIGMAS, 0, (), W)


def correlation_check(rows, rho):
    """(sample correlation, standard error, tau)"""
    x = rows[:, :2].astype(np.float64)
    r = float(np.corrcoef(x.T)[0, 1])
    tau = max(tau_sokal(x[:, 0]), tau_sokal(x[:, 1]))
    se = (1.0 - rho * rho) / math.sqrt(x.shape[0] / tau)
    return r, se, tau


def test_the_posterior_has_the_correlation_asked_for_and_none_without():
    W = sc.whitening(np.array([[1.0, RHO], [RHO, 1.0]]))
    out = {}
    for name, law, rho in (("rho = 0.9", W, RHO), ("no matrix", None, 0.0)):
        rows, accepted, ref, _ = replay_walk(nll_of(law), SEED, MEANS, initial_widths(), NSTEPS, BURNIN)
        assert rows.shape == (NSTEPS - 2 * int(NSTEPS * BURNIN), 3)
        r, se, tau = correlation_check(rows, rho)
        sd = rows[:, :2].astype(np.float64).std(axis=0)
        print("%s: acceptance %.3f, correlation %.4f, standard error %.4f (tau %.1f), %.2f standard errors off; "
              "spreads %s" % (name, accepted / NSTEPS, r, se, tau, abs(r - rho) / se, sd))
        assert abs(r - rho) <= 5.0 * se, (name, r, se)
        # the marginals are the constraints' in both: the correlation moves no width
        assert np.allclose(sd, SIGMAS, rtol=0.15), (name, sd)
        out[name] = r
    assert out["rho = 0.9"] > 0.8 and abs(out["no matrix"]) < 0.2
