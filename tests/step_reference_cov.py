"""The correlated proposal, replayed on the host.  TEST INFRASTRUCTURE ONLY.

The definition the device's step end (sxmc_group_set_proposal_factor, sxmc_launch_finish_nll_jump_pick_combo_factor)
and the host's re-tuning (sxmc_proposal_factor) are judged by.  Everything tests/step_reference.py fixes stays: the
generators, the order and the offsets of the draws, the decision, the appended row, the widths and their re-tuning.

  draws       exactly the diagonal proposal's; a fixed parameter (width <= 0) draws nothing and its z is 0
  proposal    for a free i: d_i = 0, then for j = 0 .. i ascending d_i = fma(L_ij, z_j, d_i), then v_i = cur_i + d_i,
              all in double, every operation rounded once; for a fixed i: v_i = cur_i.  The proposal drawn at set-up is
              pick_new_vector's (the diagonal law); L = diag(w) until the first re-tuning
  re-tuning   at the steps and from the kept rows of the widths' re-tuning, after it (w: the new widths, float).  With
              every float widened to double and every sum sequential in row order:
                mean_j = (sum_r x_rj) / n;  S_jk = sum_r (x_rj - mean_j)(x_rk - mean_k)
                R_jk = S_jk / (sqrt(S_jj) sqrt(S_kk)); a fixed column, one with S_jj == 0, or no rows: the identity's
                R_b: (1 - b) R_jk off the diagonal, 1 on it; b = the shrinkage option (default 0.05)
                T = Cholesky-Banachiewicz of R_b: s = A_ij; for k < j: s = s - T_ik T_jk; T_ii = sqrt(s) if s > 0, else
                    the factorisation fails; T_ij = s / T_jj
                a failure doubles b (capped at 1, where T = I) and factors again
                L_ij = (double) w_i * T_ij; rows and columns of fixed parameters are zero
              The proposal already drawn when a re-tuning happens stands.

Plain Python and numpy; nothing here is transcribed from the code under test.
"""
import math

import numpy as np

from tests.step_reference import StepReference

if hasattr(math, "fma"):
    fma = math.fma
else:
    def fma(a, b, c):
        """a * b + c rounded once: the exact rational value, rounded to nearest-even by float()."""
        a, b, c = float(a), float(b), float(c)
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
            return a * b + c
        (na, da), (nb, db), (nc, dc) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
        num = na * nb * dc + nc * da * db
        if num == 0:
            return a * b + c      # (the sign of an exact zero: as the two roundings give it)
        return num / (da * db * dc)   # (int / int is correctly rounded; the same value as float(Fraction(...)))


def diagonal_factor(jump_width):
    """L = diag(w) over the free parameters, [P, P] with L[i, j] = L_ij."""
    w = np.asarray(jump_width, np.float32)
    return np.diag(np.where(w > 0, w.astype(np.float64), 0.0))


def device_layout(L):
    """[P, P] L[i, j] -> the P * P doubles the device reads: L_ij at [j * P + i]."""
    return np.ascontiguousarray(np.asarray(L, np.float64).T).reshape(-1)


def propose_cov(z, L, jump_width, current):
    jw = np.asarray(jump_width, np.float32)
    cur = np.asarray(current, np.float64)
    out = cur.copy()
    for i in range(jw.size):
        if not jw[i] > 0:
            continue
        d = 0.0
        for j in range(i + 1):
            d = fma(float(L[i, j]), float(z[j]), d)
        out[i] = float(cur[i]) + d
    return out


def cholesky_rows(A):
    """Cholesky-Banachiewicz in double, or None at a pivot that is not positive.  (Filled column by column here, a
    column's entries at once: every entry goes through the same operations in the same order as row by row, and a
    failure anywhere fails the whole.)"""
    P = A.shape[0]
    T = np.zeros((P, P))
    for j in range(P):
        s = A[j:, j].copy()
        for k in range(j):
            s = s - T[j:, k] * T[j, k]
        if not s[0] > 0.0:
            return None
        T[j, j] = math.sqrt(s[0])
        T[j + 1:, j] = s[1:] / T[j, j]
    return T


def retune_factor(kept_rows, new_widths, shrinkage=0.05):
    """Returns (L [P, P], T [P, P], R_b [P, P], the shrinkage used)."""
    w = np.asarray(new_widths, np.float32)
    P = w.size
    rows = np.asarray(kept_rows, np.float32).reshape(-1, P + 1)[:, :P].astype(np.float64)
    n = rows.shape[0]
    free = w > 0
    S = np.zeros((P, P))
    if n > 0:
        mean = np.zeros(P)
        for r in range(n):
            mean = mean + rows[r]
        mean = mean / float(n)
        for r in range(n):
            dx = rows[r] - mean
            S = S + np.outer(dx, dx)
    coupled = free & (np.diag(S) > 0.0)
    root = np.sqrt(np.where(coupled, np.diag(S), 1.0))
    R = np.eye(P)
    for j in range(P):
        for k in range(j):
            if coupled[j] and coupled[k]:
                R[j, k] = R[k, j] = S[j, k] / (root[j] * root[k])
    b = float(shrinkage)
    while True:
        if b < 1.0:
            A = (1.0 - b) * R
            np.fill_diagonal(A, 1.0)
            T = cholesky_rows(A)
        else:
            b, A, T = 1.0, np.eye(P), np.eye(P)
        if T is not None:
            break
        b = b + b
    L = w.astype(np.float64)[:, None] * T
    L[~free, :] = 0.0
    L[:, ~free] = 0.0
    return L, T, A, b


class StepReferenceCov(StepReference):
    """StepReference with the correlated proposal: factor is L as [P, P] (L[i, j]); shrinkage_used the last b."""

    def __init__(self, *args, shrinkage=0.05, factor=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.shrinkage = float(shrinkage)
        self.shrinkage_used = None
        self.factor = diagonal_factor(self.jump_width) if factor is None else np.array(factor, np.float64)
        self.factor_history = [self.factor.copy()]

    def step(self, nll_proposed, v_proposed=None):
        rec = super().step(nll_proposed, v_proposed)      # (draws last_z and writes the diagonal proposal ...)
        self.v_proposed = propose_cov(self.last_z, self.factor, self.jump_width, self.v_current)   # ... replaced
        return rec

    def retune(self, kept_rows):
        super().retune(kept_rows)
        self.factor, _, _, self.shrinkage_used = retune_factor(kept_rows, self.jump_width, self.shrinkage)
        self.factor_history.append(self.factor.copy())


def replay_walk_cov(nll_of, seed, v0, jump_width, nsteps, burnin_fraction, debug_mode=False, proposal="covariance",
                    shrinkage=0.05):
    """tests.step_reference.replay_walk with the proposal law as an argument ("diagonal": that function's chain)."""
    burnin = int(nsteps * burnin_fraction)
    cls = {"covariance": StepReferenceCov, "diagonal": StepReference}[proposal]
    kw = dict(shrinkage=shrinkage) if proposal == "covariance" else {}
    ref = cls(seed, jump_width, v0, nll_of(np.asarray(v0, np.float64)), max(1, nsteps), debug_mode=debug_mode, **kw)
    ref.first_proposal()
    first_kept = 0
    for i in range(nsteps):
        if i == burnin or i == 2 * burnin:
            ref.retune(ref.jump_buffer[first_kept:ref.count])
            if not debug_mode:
                first_kept = ref.count
        ref.step(nll_of(ref.v_proposed))
    return ref.jump_buffer[first_kept:ref.count].copy(), ref.accepted, ref, np.arange(first_kept, ref.count)
