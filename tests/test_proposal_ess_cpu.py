"""CPU: what the correlated proposal is for, fixed without a GPU.  Both laws walk the same rates-only fit in the host
replay (tests/step_reference_cov.py, replay_walk_cov): four floated rates over one observable, of which two pairs look
alike -- unit Gaussians at 3.0 and 3.15, and at 7.0 and 7.15, 750 expected events each, 3 000 events -- so the rates of
a pair are strongly anti-correlated in the posterior.  No systematic floats: the lookup table is constant and the NLL is
numpy over events x signals (the extended likelihood of nll_total: the expected events minus the sum of the events' log
rates; a negative rate is 1e18).

Autocorrelation time by Sokal's automatic window (the smallest M with M >= 5 tau(M)) on the rows kept after the second
re-tuning; ESS = n / tau, the smallest over the floated parameters.  Asserted: the diagonal chain's |rho| of each
look-alike pair is >= 0.9, and ESS(covariance) >= 2 x ESS(diagonal) for the same seed and steps.  The floor: for a
Gaussian ridge of correlation rho the autocorrelation time of an axis-aligned proposal grows like 1 / (1 - rho^2), >= 5.3
at |rho| = 0.9; the floor of 2 is kept well below that.  Measured in the replay at this shape (seed 1, 30 000 steps,
burn-in 0.2): rho = -0.989 and -0.983; acceptance 0.104 diagonal, 0.160 covariance; tau per rate 278 / 278 / 458 / 456
against 28 / 28 / 33 / 33; ESS 39 against 550, a ratio of 14.0."""
import math

import numpy as np

from tests import step_reference_cov as cov

CENTRES = (3.0, 3.15, 7.0, 7.15)
NEVENTS, BINS, LOWER, UPPER = 3000, 40, 0.0, 10.0
NSTEPS, BURNIN, SEED = 30000, 0.2, 1


def make_nll():
    """The fit's NLL as a function of the four rates (in units of the expected 750 events each)."""
    rng = np.random.default_rng(11)
    edges = np.linspace(LOWER, UPPER, BINS + 1)
    cdf = np.array([[0.5 * (1.0 + math.erf((x - mu) / math.sqrt(2.0))) for x in edges] for mu in CENTRES])
    p = np.diff(cdf, axis=1)
    p /= p.sum(axis=1, keepdims=True)
    n = np.full(len(CENTRES), NEVENTS / len(CENTRES))
    x = np.concatenate([rng.normal(mu, 1.0, NEVENTS // len(CENTRES)) for mu in CENTRES])
    counts = np.bincount(np.clip(np.digitize(x, edges) - 1, 0, BINS - 1), minlength=BINS).astype(np.float64)
    expected = p * n[:, None]                  # per signal and bin, at rate 1
    filled = counts > 0

    def nll(v):
        v = np.asarray(v, np.float64)
        if np.any(v < 0):
            return 1e18
        return float(np.sum(v * n) - np.sum(counts[filled] * np.log((v @ expected)[filled])))
    return nll


def initial_widths():
    """mcmc.cpp:198-228 for four unconstrained rates of mean 1: 0.1 * sqrt(10) / 10 * (float)(2.4^2 / 4)."""
    ten = np.float32(10)
    return np.full(4, np.float32(0.1 * (np.sqrt(ten) / ten) * np.float32(2.4 * 2.4 / 4)), np.float32)


def tau_sokal(x, c=5.0):
    """The integrated autocorrelation time 1 + 2 sum_{t <= M} rho_t at the smallest M with M >= c tau(M)."""
    x = np.asarray(x, np.float64)
    n = x.size
    x = x - x.mean()
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    acf /= acf[0]
    tau = 1.0
    for m in range(1, n):
        tau += 2.0 * acf[m]
        if m >= c * tau:
            break
    return tau


def ess(rows):
    taus = [tau_sokal(rows[:, j]) for j in range(rows.shape[1] - 1)]
    return rows.shape[0] / max(taus), taus


def test_covariance_doubles_the_effective_sample_size_at_least():
    nll = make_nll()
    out = {}
    for law in ("diagonal", "covariance"):
        rows, accepted, ref, _ = cov.replay_walk_cov(nll, SEED, np.ones(4), initial_widths(), NSTEPS, BURNIN, proposal=law)
        assert rows.shape == (NSTEPS - 2 * int(NSTEPS * BURNIN), 5)
        n_eff, taus = ess(rows)
        rho = np.corrcoef(rows[:, :4].astype(np.float64).T)
        print("%s: acceptance %.3f, tau %s, ESS %.1f, rho(0,1) %.3f, rho(2,3) %.3f"
              % (law, accepted / NSTEPS, np.round(taus, 1), n_eff, rho[0, 1], rho[2, 3]))
        out[law] = (n_eff, rho, ref)
    rho = out["diagonal"][1]
    assert abs(rho[0, 1]) >= 0.9 and abs(rho[2, 3]) >= 0.9
    print("ESS ratio %.2f" % (out["covariance"][0] / out["diagonal"][0]))
    assert out["covariance"][0] >= 2.0 * out["diagonal"][0]
    # the marginal widths are the reference's in both laws: each row of the last factor has the width's norm
    ref = out["covariance"][2]
    L = ref.factor
    assert np.allclose(np.sqrt(np.sum(L * L, axis=1)), ref.jump_width.astype(np.float64), rtol=1e-12, atol=0)
    assert ref.shrinkage_used == 0.05 and L[1, 0] < 0 and L[3, 2] < 0        # the pairs' anti-correlation, learnt
