"""Correlated Gaussian constraints, restated on the host.  TEST INFRASTRUCTURE ONLY.

The definition the host's whitening (sxmc_constraint_whitening) and the device's constraint terms
(sxmc_group_set_constraint_whitening, sxmc_launch_finish_nll_jump_pick_combo_constrained,
sxmc_launch_nll_total_whitened) are judged by.  Everything tests/step_reference.py and tests/step_reference_cov.py fix
stays: the generators, the draws, the decision, the appended row, the widths, the proposals.  Only the NLL changes, and
of the NLL only the value of the constraint terms, not their number or their place:

  input      rho, a P x P correlation matrix over the parameter vector (sources, then <systematic>_<j>), refused when
             an entry is not finite or outside [-1, 1], a diagonal entry is not exactly 1, it is not exactly symmetric,
             or a parameter with sigma_i <= 0 has a non-zero off-diagonal entry (checked in that order)
  T          the Cholesky factor of rho, row by row, every operation one double operation:
               for i, for j = 0 .. i:  s = rho_ij;  for k = 0 .. j-1 ascending: s = s - T_ik * T_jk
                 j == i: a pivot s that is not > 0 fails "at parameter i";  T_ii = sqrt(s)
                 j <  i: T_ij = s / T_jj
  W = T^-1   by forward substitution, row by row:
               W_ii = 1 / T_ii;  for j = 0 .. i-1:  s = 0;  for k = j .. i-1 ascending: s = s + T_ik * W_kj
               W_ij = -(s * W_ii)
             a product whose T_ik is exactly zero is skipped in both loops; a W_ij all of whose products were skipped is
             +0: a parameter outside every group has W_ii = 1 and +0 beside it
  per NLL    x_i = (p_i - mean_i) / sigma_i for sigma_i > 0, else 0
             r_i = 0, then for j = 0 .. i ascending r_i = fma(W_ij, x_j, r_i)
             pen_i = 0.5 * r_i * r_i for sigma_i > 0, else -0.0
             nll = -event sum; + every signal's expected-rate term in order; + pen_0, + pen_1, ... in order (the slots the
             independent constraints have, nll_kernels.cpp:166-186); 1e18 on a NaN event sum or a negative source rate

THE ACCURACY BOUND (accuracy_bound below).  u = 2^-53, gamma(n) = n u / (1 - n u), kappa = the 2-norm condition number
of rho.  The computed factor satisfies That That^T = rho + D with |D| <= gamma(P + 1) |That| |That^T| (Higham, Accuracy
and Stability of Numerical Algorithms, thm 10.3), and since the rows of T have unit norm, ||D||_F <= gamma(P + 1) P.
Each column of What solves a triangular system by substitution, backward stable with |dT| <= gamma(P) |That| (thm 8.5),
and the product rhat = fl(What x) has the forward error gamma(P) |What| |x| (fma sums do no worse than plain ones).
So rhat = (T + E)^-1 x up to first order with ||E||_F / ||T||_2 <= [gamma(P + 1) P kappa / 2 + 2 gamma(P) sqrt(P)]:
the first term is the perturbation of a Cholesky factor under a perturbation of its matrix (Sun 1991; Higham sec 10.3:
||dT||_F / ||T||_2 <= kappa ||D||_F / (sqrt(2) ||rho||_2 ) and ||rho||_2 >= 1), the others the two triangular steps (a
row of unit norm in P entries: sqrt(P)).  The relative change of r is at most kappa(T) = sqrt(kappa) times that, the
relative change of q = 0.5 r.r twice that of r, and forming q itself adds gamma(P + 2).  Altogether

    |qhat - q| / q  <=  2 sqrt(kappa) [gamma(P + 1) P kappa / 2 + 2 gamma(P) sqrt(P)] + gamma(P + 2).

The tests allow twice this, as the cross-validation tests do with their bound.

Plain Python and numpy; nothing here is transcribed from the code under test.
"""
import math

import numpy as np

from tests.step_reference import StepReference
from tests.step_reference_cov import StepReferenceCov, fma

U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the input
def refusal(rho, sigmas):
    """None for an accepted matrix, else (kind, i, j): 'range', 'diagonal', 'symmetry' or 'unconstrained'."""
    rho = np.asarray(rho, np.float64)
    P = rho.shape[0]
    for i in range(P):
        for j in range(P):
            v = rho[i, j]
            if not math.isfinite(v) or v < -1.0 or v > 1.0:
                return "range", i, j
    for i in range(P):
        if rho[i, i] != 1.0:
            return "diagonal", i, i
    for i in range(P):
        for j in range(i):
            if rho[i, j] != rho[j, i]:
                return "symmetry", i, j
    for i in range(P):
        if sigmas[i] > 0:
            continue
        for j in range(P):
            if j != i and rho[i, j] != 0.0:
                return "unconstrained", i, j
    return None


# ------------------------------------------------------------------------------------------------ the whitening
def cholesky_rows(rho):
    """(T, None), or (None, i) at the first pivot that is not positive.  Filled column by column, a column's entries at
    once: every entry goes through the operations above in their order (k ascending), and the first pivot to fail is
    the same.  Products with an exactly zero T_ik are not skipped here: subtracting an exact zero changes nothing but
    the sign of a zero, which nothing below reads."""
    rho = np.asarray(rho, np.float64)
    P = rho.shape[0]
    T = np.zeros((P, P))
    for j in range(P):
        s = rho[j:, j].copy()
        for k in range(j):
            s = s - T[j:, k] * T[j, k]
        if not s[0] > 0.0:
            return None, j
        T[j, j] = math.sqrt(s[0])
        T[j + 1:, j] = s[1:] / T[j, j]
    return T, None


def inverse_rows(T):
    """Row i at once: entry j takes its products for k = j .. i-1 ascending.  A sum that starts at +0 is never -0, so
    the products of an exactly zero T_ik change nothing; the entries ALL of whose products have one are set to +0."""
    P = T.shape[0]
    W = np.zeros((P, P))
    for i in range(P):
        inverse = 1.0 / T[i, i]
        W[i, i] = inverse
        nz = np.flatnonzero(T[i, :i])
        if nz.size == 0:
            continue
        s = np.zeros(i)
        for k in range(i):
            s[:k + 1] = s[:k + 1] + T[i, k] * W[k, :k + 1]
        live = nz[-1] + 1                     # j <= the last k with T_ik != 0
        W[i, :live] = -(s[:live] * inverse)
    return W


def whitening(rho):
    """W as [P, P] (W[i, j] = W_ij); raises ValueError naming the pivot for a matrix that is not positive definite."""
    T, bad = cholesky_rows(rho)
    if T is None:
        raise ValueError("not positive definite at parameter %d" % bad)
    return inverse_rows(T)


def device_layout(W):
    """[P, P] W[i, j] -> the P * P doubles the device reads: W_ij at [j * P + i]."""
    return np.ascontiguousarray(np.asarray(W, np.float64).T).reshape(-1)


# ------------------------------------------------------------------------------------------------ the NLL's terms
def residuals(p, means, sigmas):
    p, means, sigmas = (np.asarray(a, np.float64) for a in (p, means, sigmas))
    x = np.zeros(p.size)
    c = sigmas > 0
    with np.errstate(all="ignore"):
        x[c] = (p[c] - means[c]) / sigmas[c]
    return x


def whitened(W, x):
    P = x.size
    r = np.zeros(P)
    for i in range(P):
        acc = 0.0
        for j in range(i + 1):
            acc = fma(float(W[i, j]), float(x[j]), acc)
        r[i] = acc
    return r


def penalties(p, means, sigmas, W=None):
    """pen_i in slot order; W None: the independent constraints (nll_kernels.cpp:181-184)."""
    x = residuals(p, means, sigmas)
    r = x if W is None else whitened(W, x)
    with np.errstate(all="ignore"):
        pen = 0.5 * r * r
    pen[~(np.asarray(sigmas, np.float64) > 0)] = -0.0
    return pen


def nll_total(event_sum, p, means, sigmas, nsources, signal_terms=(), W=None, pens=None):
    """nll_total (nll_kernels.cpp:160-189) with the constraint terms above, every addition in the reference's order."""
    s = -np.float64(event_sum)
    if math.isnan(s):
        return 1e18
    with np.errstate(all="ignore"):
        for t in signal_terms:
            s = s + np.float64(t)
        if any(float(v) < 0 for v in np.asarray(p, np.float64)[:nsources]):
            return 1e18
        for t in (penalties(p, means, sigmas, W) if pens is None else pens):
            s = s + np.float64(t)
    return float(s)


# -- planted wrong laws: each must be told from the law above by the tests that hold the device to it
def penalties_with_T(p, means, sigmas, rho):
    """W = T instead of T^-1."""
    return penalties(p, means, sigmas, cholesky_rows(rho)[0])


def penalties_descending(p, means, sigmas, W):
    """The product taken descending in j."""
    x = residuals(p, means, sigmas)
    r = np.zeros(x.size)
    for i in range(x.size):
        acc = 0.0
        for j in range(i, -1, -1):
            acc = fma(float(W[i, j]), float(x[j]), acc)
        r[i] = acc
    pen = 0.5 * r * r
    pen[~(np.asarray(sigmas, np.float64) > 0)] = -0.0
    return pen


def nll_total_extra_term(event_sum, p, means, sigmas, nsources, signal_terms, W):
    """The penalty added as ONE extra term at the end (the slots hold -0.0)."""
    pens = penalties(p, means, sigmas, W)
    q = np.float64(0.0)
    for t in pens:
        q = q + t
    s = nll_total(event_sum, p, means, sigmas, nsources, signal_terms, pens=np.full(pens.size, -0.0))
    return float(np.float64(s) + q)


def penalties_sigma_after(p, means, sigmas, W):
    """sigma applied after the product: r = W (p - mean), then divided by sigma_i."""
    p, means, sigmas = (np.asarray(a, np.float64) for a in (p, means, sigmas))
    d = np.where(sigmas > 0, p - means, 0.0)
    r = whitened(W, d)
    with np.errstate(all="ignore"):
        r = np.where(sigmas > 0, r / np.where(sigmas > 0, sigmas, 1.0), 0.0)
        pen = 0.5 * r * r
    pen[~(sigmas > 0)] = -0.0
    return pen


# ------------------------------------------------------------------------------------------------ accuracy
def gamma(n):
    return n * U / (1.0 - n * U)


def accuracy_bound(rho):
    """The relative bound on 0.5 sum r_i^2 against 0.5 x^T rho^-1 x derived in this file's docstring."""
    rho = np.asarray(rho, np.float64)
    P = rho.shape[0]
    ev = np.linalg.eigvalsh(rho)
    kappa = float(ev[-1] / ev[0])
    return 2.0 * math.sqrt(kappa) * (gamma(P + 1) * P * kappa / 2.0 + 2.0 * gamma(P) * math.sqrt(P)) + gamma(P + 2)


def quadratic_form_longdouble(rho, x):
    """0.5 x^T rho^-1 x with rho^-1 x solved in np.longdouble (Gaussian elimination with partial pivoting)."""
    A = np.array(rho, np.longdouble)
    b = np.array(x, np.longdouble)
    n = b.size
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
            b[[c, piv]] = b[[piv, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:, c:] -= f[:, None] * A[c, c:][None, :]
        b[c + 1:] -= f * b[c]
    y = np.zeros(n, np.longdouble)
    for c in range(n - 1, -1, -1):
        y[c] = (b[c] - A[c, c + 1:] @ y[c + 1:]) / A[c, c]
    return np.longdouble(0.5) * (np.array(x, np.longdouble) @ y)


# ------------------------------------------------------------------------------------------------ cases
def block_matrix(P, blocks):
    """The P x P identity with blocks [(indices, matrix), ...] scattered in."""
    rho = np.eye(P)
    for idx, m in blocks:
        idx = np.asarray(idx)
        rho[np.ix_(idx, idx)] = np.asarray(m, np.float64)
    return rho


def random_correlation(P, rng, strength=0.6):
    """A dense, well-conditioned correlation matrix, exactly symmetric with an exact unit diagonal."""
    k = max(2, P // 4)
    f = rng.standard_normal((P, k)) * strength / math.sqrt(k)
    c = f @ f.T
    c = c + np.diag(1.0 - np.diag(c).clip(max=0.9))
    d = np.sqrt(np.diag(c))
    c = c / d[:, None] / d[None, :]
    c = np.clip(np.tril(c, -1), -1.0, 1.0)
    c = c + c.T
    np.fill_diagonal(c, 1.0)
    return c


# ------------------------------------------------------------------------------------------------ walks
def replay_walk_constrained(nll_of, seed, v0, jump_width, nsteps, burnin_fraction, debug_mode=False,
                            proposal="diagonal", shrinkage=0.05):
    """tests.step_reference.replay_walk; the constraints are in nll_of.  Kept here so that tests of this feature need
    one import."""
    from tests.step_reference_cov import replay_walk_cov
    return replay_walk_cov(nll_of, seed, v0, jump_width, nsteps, burnin_fraction, debug_mode, proposal, shrinkage)


__all__ = ["StepReference", "StepReferenceCov"]
