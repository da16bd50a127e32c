"""What correlated constraints are for, once on the device: the chain of tests/test_constraint_posterior_cpu.py -- two
parameters the likelihood does not depend on, rho = 0.9 between their constraints -- at the smallest fit that has two
such parameters: the step end alone (sxmc_launch_finish_nll_jump_pick_combo_constrained; one signal of expected rate 0,
event sums of 0), 30 000 steps with the walk's two re-tunings.  The kept rows' sample correlation must lie within 5
standard errors of 0.9; with no matrix, of 0.  The device's deviates differ from the host's in their last bits, so the
chains are not compared row by row: the step end's law is held to the replay as bytes in
tests/test_gpu_constraint_step_end.py."""
import numpy as np
import pytest

from sxmc_amd import capi
from sxmc_amd.capi import DeviceArray
from tests import step_reference_constraints as sc
from tests.test_constraint_posterior_cpu import (BURNIN, MEANS, NSTEPS, RHO, SIGMAS, correlation_check,
                                                 initial_widths)
from tests.test_gpu_constraint_step_end import Chain, on_device

pytestmark = pytest.mark.gpu


def device_walk(W):
    widths = initial_widths()
    c = Chain(2, 0, MEANS, SIGMAS, widths, MEANS, 0.0, NSTEPS)
    c.nexpected = DeviceArray(np.zeros(1))                      # the signal's term is p_0 * 0: the likelihood is flat
    d_W = on_device(W) if W is not None else None
    c.first_proposal()
    b = int(NSTEPS * BURNIN)
    scale = float(np.float32(2.4 * 2.4 / 2))
    args = c.args(128, 0.0) + [capi.ptr(None), capi.ptr(d_W)]
    lib_call = capi.call
    for i in range(NSTEPS):
        if i in (b, 2 * b):                                     # mcmc.cpp:274-311 over the rows since the last re-tuning
            capi.synchronize()
            rows = c.jb.get().reshape(NSTEPS, 3)[i - b:i, :2].astype(np.float64)
            c.jw.set((scale * rows.std(axis=0)).astype(np.float32))
        lib_call("sxmc_launch_finish_nll_jump_pick_combo_constrained", *args)
    capi.synchronize()
    assert int(c.cnt.get()[0]) == NSTEPS
    return c.jb.get().reshape(NSTEPS, 3)[2 * b:], int(c.acc.get()[0])


@pytest.mark.parametrize("name,rho", [("rho = 0.9", RHO), ("no matrix", 0.0)])
def test_the_posterior_on_the_device_has_the_correlation_asked_for(name, rho):
    W = sc.whitening(np.array([[1.0, rho], [rho, 1.0]])) if rho else None
    rows, accepted = device_walk(W)
    r, se, tau = correlation_check(rows, rho)
    sd = rows[:, :2].astype(np.float64).std(axis=0)
    print("%s: acceptance %.3f, correlation %.4f, standard error %.4f (tau %.1f), %.2f standard errors off; spreads %s"
          % (name, accepted / NSTEPS, r, se, tau, abs(r - rho) / se, sd))
    assert abs(r - rho) <= 5.0 * se, (name, r, se)
    assert np.allclose(sd, SIGMAS, rtol=0.15), sd
    # the last column is the NLL: the constraints' alone, 0.5 x^T rho^-1 x, never negative and about one on average
    assert np.all(rows[:, 2] >= 0.0) and 0.7 < float(rows[:, 2].mean()) < 1.3
