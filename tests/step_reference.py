"""The end of an MCMC step, replayed on the host.  TEST INFRASTRUCTURE ONLY.

What a step end does is fixed by the reference (src/nll_kernels.cpp:30-86 pick_new_vector / jump_decider, :230-271 their
fused form, src/mcmc.cpp:198-311 the set-up draw and the two re-tunings); the random law is this project's own (README,
"Random numbers"; sxmc_amd/csrc/nll_device.h), because the reference's cuRAND stream cannot be reproduced:

  generator i   Philox4x32-10, key = the seed, counter words = (offset low, offset high, i low, i high); the offset
                advances by one per draw
  uniform       (word0 + 1) * 2^-32, in (0, 1]
  normal        sqrt(-2 ln((word0 + 1) * 2^-32)) * cos(6.283185307179586 * word1 * 2^-32), in double
  order         at set-up one normal from every FREE parameter's generator (free: jump width > 0); then, per step,
                generator 0 hands the decider its uniform -- also when parameter 0 is fixed -- and after it every free
                parameter's generator one normal

Plain Python and numpy.  NLL values are not computed here: the caller takes them from the CPU oracle (oracle.full_nll
or oracle_nll_of_workload) and hands them in.  Nothing here is transcribed from the device's step end: the device is
what this file judges (tests/test_gpu_step_replay.py; tests/test_step_reference_cpu.py pins this file to the C oracle's
jump_decider / pick_new_vector and to the Random123 known answers).
"""
import math

import numpy as np

from tests.helpers import philox4x32_10

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
TWO_PI = 6.283185307179586


# ---------------------------------------------------------------------------------------------- the random law
def generator_words(seed, index, offset):
    """The four words of draw `offset` of generator `index` under `seed` (each a 64-bit integer)."""
    return philox4x32_10((offset & M32, (offset >> 32) & M32, index & M32, (index >> 32) & M32),
                         (seed & M32, (seed >> 32) & M32))


def word_to_uniform(word0):
    return (word0 + 1) * 2.0 ** -32


def words_to_normal(word0, word1):
    return math.sqrt(-2.0 * math.log((word0 + 1) * 2.0 ** -32)) * math.cos(TWO_PI * (word1 * 2.0 ** -32))


# ---------------------------------------------------------------------------------------------- the transition
def decide(u, nll_current, nll_proposed, debug_mode=False):
    """Metropolis, nll_kernels.cpp:69-71.  (`or` does not evaluate the exponential of a downhill step, which may overflow;
    inf - inf is NaN, its exponential NaN, and no u is <= NaN: a rejection.)"""
    return bool(debug_mode or nll_proposed < nll_current or u <= math.exp(nll_current - nll_proposed))


def margin_of(u, nll_current, nll_proposed):
    """For an uphill decision (one the uniform decides): |u - e| / e with e = exp(nc - np), how far in relative terms
    the exponential would have to move to change the decision.  inf where e is 0 or NaN (a proposal at +inf or 1e18 from
    a finite value, inf - inf): no rounding of an NLL moves those.  None for a downhill step."""
    if nll_proposed < nll_current:
        return None
    e = math.exp(nll_current - nll_proposed)
    if not e > 0.0:
        return math.inf
    return abs(u - e) / e


def propose(z, jump_width, current):
    """nll_kernels.cpp:38-51, device form: current + width * z for the free parameters, current for the fixed ones
    (width -1, mcmc.cpp:204-207).  The float width is widened to double before the product."""
    jw = np.asarray(jump_width, np.float32)
    cur = np.asarray(current, np.float64)
    z = np.asarray(z, np.float64)
    out = cur.copy()
    free = jw > 0
    out[free] = cur[free] + jw[free].astype(np.float64) * z[free]
    return out


class StepReference:
    """One chain's state and its step end.  jump_buffer is the device's buffer as a [nrows, P + 1] float32 array
    (rows that no step has written keep `fill`); offsets[i] is generator i's offset."""

    def __init__(self, seed, jump_width, v_current, nll_current, nrows, offsets=None, accepted=0, count=0,
                 debug_mode=False, fill=0.0):
        self.seed = int(seed)
        self.jump_width = np.array(jump_width, np.float32)
        self.P = self.jump_width.size
        self.v_current = np.array(v_current, np.float64)
        assert self.v_current.size == self.P
        self.nll_current = float(nll_current)
        self.v_proposed = self.v_current.copy()
        self.offsets = [0] * self.P if offsets is None else [int(o) for o in offsets]
        self.accepted, self.count = int(accepted), int(count)
        self.debug_mode = bool(debug_mode)
        self.jump_buffer = np.full((nrows, self.P + 1), fill, np.float32)
        self.decisions = []          # per step: dict(u, accept, uphill, margin, nll_current, nll_proposed)
        self.last_z = np.zeros(self.P)
        self.width_history = [self.jump_width.copy()]      # the widths of every stretch of the walk

    # -- draws
    def _next_words(self, i):
        w = generator_words(self.seed, i, self.offsets[i])
        self.offsets[i] = (self.offsets[i] + 1) & M64
        return w

    def draw_uniform(self):
        return word_to_uniform(self._next_words(0)[0])

    def draw_normals(self):
        z = np.zeros(self.P)
        for i in range(self.P):
            if self.jump_width[i] > 0:
                w = self._next_words(i)
                z[i] = words_to_normal(w[0], w[1])
        return z

    # -- mcmc.cpp:252-256, the proposal drawn at set-up
    def first_proposal(self):
        self.last_z = self.draw_normals()
        self.v_proposed = propose(self.last_z, self.jump_width, self.v_current)
        return self.v_proposed

    # -- nll_kernels.cpp:230-271: decide, append, propose
    def step(self, nll_proposed, v_proposed=None):
        """One step end with `nll_proposed` the NLL at the proposed vector.  v_proposed: decide on THIS vector instead of
        the reference's own proposal (a test that follows a device hands in the device's, which it has checked against
        self.v_proposed first).  Returns the decision's record."""
        if v_proposed is not None:
            self.v_proposed = np.array(v_proposed, np.float64)
        np_, nc = float(nll_proposed), self.nll_current
        u = self.draw_uniform()
        accept = decide(u, nc, np_, self.debug_mode)
        rec = dict(u=u, accept=accept, uphill=not np_ < nc, margin=margin_of(u, nc, np_), nll_current=nc,
                   nll_proposed=np_)
        self.decisions.append(rec)
        if accept:
            self.v_current = self.v_proposed.copy()
            self.nll_current = np_
            self.accepted += 1
        with np.errstate(over="ignore"):
            self.jump_buffer[self.count, :self.P] = self.v_current.astype(np.float32)
            self.jump_buffer[self.count, self.P] = np.float32(self.nll_current)
        self.count += 1
        self.last_z = self.draw_normals()
        self.v_proposed = propose(self.last_z, self.jump_width, self.v_current)
        return rec

    # -- mcmc.cpp:274-311
    def retune(self, kept_rows):
        """New widths from the rows kept so far: (float)(2.4^2 / nfloat) times the standard deviation of each free
        parameter's column (taken in double, as TH1::GetRMS does), the old width where that is 0.  The proposal already
        drawn with the old widths stands: it is the one the next step evaluates."""
        free = self.jump_width > 0
        scale = float(np.float32(2.4 * 2.4 / max(1, int(np.count_nonzero(free)))))
        rows = np.asarray(kept_rows, np.float32).reshape(-1, self.P + 1).astype(np.float64)
        for j in range(self.P):
            if not free[j]:
                continue
            sd = float(rows[:, j].std()) if rows.shape[0] > 0 else 0.0
            fit_width = sd if sd > 0 else float(self.jump_width[j])
            self.jump_width[j] = np.float32(scale * fit_width)
        self.width_history.append(self.jump_width.copy())

    # -- summaries for the conditions the tests put on a chain
    def summary(self):
        d = self.decisions
        margins = [r["margin"] for r in d if r["uphill"]]
        return dict(steps=len(d), accepted=sum(r["accept"] for r in d),
                    rejections=sum(not r["accept"] for r in d),
                    uphill_accepted=sum(r["accept"] and r["uphill"] for r in d),
                    min_margin=min(margins) if margins else math.inf)


def replay_walk(nll_of, seed, v0, jump_width, nsteps, burnin_fraction, debug_mode=False):
    """MCMC::operator() (mcmc.cpp:143-387) with every NLL from nll_of(vector): start at v0, first proposal, nsteps steps,
    re-tuning at i == burnin and i == 2 * burnin from the rows kept so far, which are then dropped unless in debug
    mode.  Returns (kept rows [nkept, P + 1] float32, accepted steps of the whole walk, the StepReference, and for
    each kept row the index of its step)."""
    burnin = int(nsteps * burnin_fraction)
    ref = StepReference(seed, jump_width, v0, nll_of(np.asarray(v0, np.float64)), max(1, nsteps),
                        debug_mode=debug_mode)
    ref.first_proposal()
    first_kept = 0
    for i in range(nsteps):
        if i == burnin or i == 2 * burnin:
            ref.retune(ref.jump_buffer[first_kept:ref.count])
            if not debug_mode:
                first_kept = ref.count
        ref.step(nll_of(ref.v_proposed))
    return ref.jump_buffer[first_kept:ref.count].copy(), ref.accepted, ref, np.arange(first_kept, ref.count)
