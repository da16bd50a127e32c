"""The correlated proposal in the step end alone: sxmc_launch_finish_nll_jump_pick_combo_factor with handed-in sums,
step by step beside the host replay (tests/step_reference_cov.py), as bytes.

WHAT IS COMPARED AS BYTES, AND HOW.  The replay's normal deviates come from the host's log and cos, the device's from
its own: they agree to 1e-12 (the project's bound, tests/test_gpu_step_replay.py), not to the bit, and no law of the
product can be read off vectors that differ in their inputs.  So the device's own deviates are read from the device,
through code this change does not touch: a TWIN chain with the same generators walks beside the chain under test through
the existing launch point, with current vector 0, widths of exactly 1 and sums that refuse every step -- its v_proposed
is 0 + 1 * z = z.  The twin's z is held to the replay's own draw within that bound and then handed to the replay, whose
product L z -- exact arithmetic rounded once per term -- must be the device's v_proposed bit for bit, with every
jump-buffer row, both counters, the current vector and NLL, and every generator's offset.

The NLL is handed in: one partial sum per step, one signal of expected rate 0 and no constraint, so the NLL of a step
is the negated sum exactly; the sums are chosen so that steps are accepted downhill, accepted uphill and refused.
The factor is dense and random; everything above its diagonal is NaN (it must never be read), and the columns of fixed
parameters are not zero (their z is)."""
import numpy as np
import pytest

from sxmc_amd import capi, nll
from sxmc_amd.capi import DeviceArray
from tests import step_reference_cov as cov

pytestmark = pytest.mark.gpu

NSTEPS = 40
FILL = -7.5
SEED = 20240613
# P, fixed parameters, lanes of the workgroup: one wave, one and a half, two (the walk's), sixteen; 255 and 256
# parameters in 128 lanes are two rounds of the staging loops
# fixed parameters in the middle (5 and 9 of 17; a run of them ahead of the last lanes of 256): their z is 0 whatever the
# factor's column holds, and the free parameters behind them read it
CASES = [(1, (), 128), (2, (), 64), (17, (0,), 128), (17, (16,), 96), (17, (5, 9), 128), (17, (1, 2, 3), 64),
         (255, (254,), 1024), (256, (), 128), (256, (100, 101, 200), 128)]


class Chain:
    def __init__(self, P, fixed, v0, widths, nll0):
        self.P = P
        w = np.array(widths, np.float32)
        self.d = dict(means=DeviceArray(np.zeros(P)), sigmas=DeviceArray(np.zeros(P)),
                      nexpected=DeviceArray(np.zeros(1)), n_mc=DeviceArray(np.ones(1, np.uint32)),
                      norms=DeviceArray(np.ones(1, np.uint32)), source_id=DeviceArray(np.zeros(1, np.int16)))
        self.jw = DeviceArray(w)
        self.rngs = nll.make_rngs(P, SEED)
        self.v_cur, self.v_prop = DeviceArray(np.array(v0, np.float64)), DeviceArray(np.full(P, np.nan))
        self.nll_cur, self.nll_prop = DeviceArray(np.array([nll0])), DeviceArray.zeros(1, np.float64)
        self.acc, self.cnt = DeviceArray.zeros(1, np.int32), DeviceArray.zeros(1, np.int32)
        self.nrows = NSTEPS + 1
        self.jb = DeviceArray(np.full(self.nrows * (P + 1), FILL, np.float32))
        self.sum = DeviceArray.zeros(1, np.float64)
        capi.synchronize()

    def first_proposal(self):
        nll.pick_new_vector(1, 64, None, self.P, self.rngs, self.jw, self.v_cur, self.v_prop)

    def args(self, block, total):
        self.sum.set(np.array([total]))
        d = self.d
        return [1, block, capi.ptr(None), 1, capi.ptr(self.sum), 1, 0, capi.ptr(d["means"]), capi.ptr(d["sigmas"]),
                capi.ptr(self.rngs), capi.ptr(self.nll_cur), capi.ptr(self.nll_prop), capi.ptr(self.v_cur),
                capi.ptr(self.v_prop), capi.ptr(self.acc), capi.ptr(self.cnt), capi.ptr(self.jb), self.P,
                capi.ptr(self.jw), capi.ptr(d["nexpected"]), capi.ptr(d["n_mc"]), capi.ptr(d["source_id"]),
                capi.ptr(d["norms"]), 0]

    def step(self, block, total, factor):
        """factor: a DeviceArray, or None for the launch point that was there before."""
        if factor is None:
            capi.call("sxmc_launch_finish_nll_jump_pick_combo", *self.args(block, total))
        else:
            capi.call("sxmc_launch_finish_nll_jump_pick_combo_factor", *self.args(block, total), capi.ptr(factor))

    def offsets(self):
        st = self.rngs.get().reshape(self.P, 4)
        return [int(o) for o in st[:, 2]]

    def state(self):
        capi.synchronize()
        return b"".join(a.get().tobytes() for a in (self.v_cur, self.v_prop, self.nll_cur, self.nll_prop, self.acc,
                                                    self.cnt, self.jb, self.rngs))


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[np.asarray(a).dtype.itemsize])


def make(P, fixed):
    rng = np.random.default_rng(1000 + P + 7 * len(fixed) + sum(fixed))
    widths = (0.02 + 0.05 * rng.random(P)).astype(np.float32)
    widths[list(fixed)] = -1.0
    v0 = 50.0 + rng.standard_normal(P)
    L = np.tril(0.05 * rng.standard_normal((P, P)) / np.sqrt(np.arange(1, P + 1))[:, None])
    L[np.triu_indices(P, 1)] = np.nan
    return widths, v0, L


def handed_in_nlls(rng, n):
    """NLLs around 100: most steps are decided by the uniform, some go downhill, some far uphill."""
    return 100.0 + rng.choice([0.3, 1.0, 6.0], size=n) * rng.standard_normal(n)


@pytest.mark.parametrize("P,fixed,block", CASES)
def test_step_end_with_a_dense_factor_equals_the_replay_as_bytes(P, fixed, block):
    widths, v0, L = make(P, fixed)
    free = widths > 0
    factor = DeviceArray(cov.device_layout(L))
    nlls = handed_in_nlls(np.random.default_rng(P), NSTEPS)
    c = Chain(P, fixed, v0, widths, 100.0)
    twin = Chain(P, fixed, np.zeros(P), np.where(free, 1.0, -1.0), 0.0)
    ref = cov.StepReferenceCov(SEED, widths, v0, 100.0, c.nrows, fill=FILL, factor=np.nan_to_num(L, nan=0.0))
    c.first_proposal()
    twin.first_proposal()
    ref.first_proposal()
    capi.synchronize()
    # the set-up's proposal is pick_new_vector's, the diagonal law: within the bound on a device normal
    z = twin.v_prop.get()
    assert np.all(np.abs(z - ref.last_z) <= 8e-12) and np.all(z[~free] == 0.0)
    assert np.all(np.abs(c.v_prop.get() - ref.v_proposed) <= 8e-12 * np.abs(widths) + 2.0 ** -52 * np.abs(ref.v_proposed))
    ref.v_proposed = c.v_prop.get()
    accepted = 0
    for k in range(NSTEPS):
        c.step(block, -nlls[k], factor)
        twin.step(block, -1e300, None)          # NLL 1e300 against 0: refused, the twin's current vector stays 0
        capi.synchronize()
        assert bits(c.nll_prop.get())[0] == bits(np.array([nlls[k]]))[0], k
        rec = ref.step(nlls[k])
        accepted += rec["accept"]
        z = twin.v_prop.get()
        assert int(twin.acc.get()[0]) == 0 and np.all(twin.v_cur.get() == 0.0)
        assert np.all(np.abs(z - ref.last_z) <= 8e-12), k
        assert np.all(z[~free] == 0.0)
        ref.last_z = z
        ref.v_proposed = cov.propose_cov(z, ref.factor, widths, ref.v_current)
        assert np.array_equal(bits(c.v_prop.get()), bits(ref.v_proposed)), (k, np.flatnonzero(
            bits(c.v_prop.get()) != bits(ref.v_proposed))[:4])
        assert np.array_equal(bits(c.v_cur.get()), bits(ref.v_current)), k
        assert bits(c.nll_cur.get())[0] == bits(np.array([ref.nll_current]))[0], k
        assert (int(c.acc.get()[0]), int(c.cnt.get()[0])) == (ref.accepted, ref.count) == (accepted, k + 1)
        assert np.array_equal(bits(c.jb.get().reshape(c.nrows, P + 1)), bits(ref.jump_buffer)), k
        assert c.offsets() == ref.offsets == twin.offsets(), k
    uphill = sum(r["accept"] and r["uphill"] for r in ref.decisions)
    print("P=%d: %d of %d accepted, %d of them uphill" % (P, accepted, NSTEPS, uphill))
    assert 0 < accepted < NSTEPS
    if free.any():
        moved = ref.jump_buffer[:NSTEPS, :P].astype(np.float64) - v0.astype(np.float32)
        assert np.all(moved[:, ~free] == 0.0) and np.any(moved[:, free] != 0.0)


@pytest.mark.parametrize("P", [257, 300])
def test_a_factor_beyond_the_staged_form_is_refused(P):
    widths, v0, _ = make(P, ())
    c = Chain(P, (), v0, widths, 100.0)
    factor = DeviceArray.zeros(P * P, np.float64)
    c.first_proposal()
    before = c.state()
    with pytest.raises(capi.SxmcError) as e:
        c.step(128, -100.0, factor)
    assert e.value.code == capi.ERR_SHAPE and "256 parameters" in e.value.msg
    assert c.state() == before                                   # nothing was launched
    c.step(128, -100.0, 0)                                       # a null factor: the unstaged form, as ever
    capi.synchronize()
    assert int(c.cnt.get()[0]) == 1


@pytest.mark.parametrize("P,fixed,block", [(1, (), 128), (17, (0,), 96), (256, (), 128), (300, (3,), 128)])
def test_a_null_factor_is_the_existing_launch_point_as_bytes(P, fixed, block):
    widths, v0, _ = make(P, fixed)
    nlls = handed_in_nlls(np.random.default_rng(P), 12)
    a, b = Chain(P, fixed, v0, widths, 100.0), Chain(P, fixed, v0, widths, 100.0)
    a.first_proposal()
    b.first_proposal()
    for k in range(12):
        a.step(block, -nlls[k], None)
        b.step(block, -nlls[k], 0)              # the new launch point, d_factor = NULL
    assert a.state() == b.state()
    assert 0 < int(a.acc.get()[0]) < 12
