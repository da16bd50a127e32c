"""Correlated constraints in the step end alone: sxmc_launch_finish_nll_jump_pick_combo_constrained with handed-in event
sums, step by step beside the host replay, as bytes.

The NLL a step decides on is formed on the device from the proposal it finds, and that proposal is read back before the
step: the replay (tests/step_reference_constraints.py) forms the same NLL from the same doubles -- the negated event sum,
one signal's expected-rate term, then every constraint's 0.5 r_i^2 in its slot -- and the device's must be that number's
bits.  From there on the chain is compared as in tests/test_gpu_proposal_step_end.py: a TWIN chain through the launch
point that was there before hands over the device's own normal deviates (held to the replay's within the project's bound
on a device normal), and every proposal, jump-buffer row, counter and generator offset must be the replay's bytes, with
the diagonal proposal and with a dense proposal factor.

The whitening matrix is the library's own (sxmc_constraint_whitening, held to the restatement in
tests/test_constraint_whitening_cpu.py) of a dense correlation matrix over the constrained parameters; everything above
its diagonal is NaN on the device (it must never be read).  Unconstrained parameters (sigma 0 or negative) and fixed
ones (width -1) stand between the others; a fixed parameter takes part in the correlations."""
import numpy as np
import pytest

from sxmc_amd import capi, nll
from sxmc_amd.capi import DeviceArray
from tests import step_reference_constraints as sc
from tests import step_reference_cov as cov

pytestmark = pytest.mark.gpu

FILL = -7.5
SEED = 20250317
NEXPECTED, NORM, N_MC = 2.5, 3, 7
# P, fixed parameters, unconstrained parameters, lanes of the workgroup (one wave, one and a half, two, sixteen; 255 and
# 256 parameters in 128 lanes are two rounds of every staging loop), steps
CASES = [(1, (), (), 128, 24), (2, (), (), 64, 24), (17, (5, 9), (0, 12), 128, 24), (17, (0,), (16,), 96, 24),
         (255, (254,), (3, 100), 1024, 6), (256, (100, 101, 200), (0, 255), 128, 6)]


class Chain:
    def __init__(self, P, nsources, means, sigmas, widths, v0, nll0, nrows):
        self.P, self.nsources = P, nsources
        self.means, self.sigmas = DeviceArray(np.array(means, np.float64)), DeviceArray(np.array(sigmas, np.float64))
        self.nexpected = DeviceArray(np.array([NEXPECTED]))
        self.n_mc, self.norms = DeviceArray(np.array([N_MC], np.uint32)), DeviceArray(np.array([NORM], np.uint32))
        self.source_id = DeviceArray(np.zeros(1, np.int16))
        self.jw = DeviceArray(np.array(widths, np.float32))
        self.rngs = nll.make_rngs(P, SEED)
        self.v_cur, self.v_prop = DeviceArray(np.array(v0, np.float64)), DeviceArray(np.full(P, np.nan))
        self.nll_cur, self.nll_prop = DeviceArray(np.array([nll0])), DeviceArray.zeros(1, np.float64)
        self.acc, self.cnt = DeviceArray.zeros(1, np.int32), DeviceArray.zeros(1, np.int32)
        self.nrows = nrows
        self.jb = DeviceArray(np.full(nrows * (P + 1), FILL, np.float32))
        self.sum = DeviceArray.zeros(1, np.float64)
        capi.synchronize()

    def first_proposal(self):
        nll.pick_new_vector(1, 64, None, self.P, self.rngs, self.jw, self.v_cur, self.v_prop)

    def args(self, block, total):
        self.sum.set(np.array([total]))
        p = capi.ptr
        return [1, block, p(None), 1, p(self.sum), 1, self.nsources, p(self.means), p(self.sigmas), p(self.rngs),
                p(self.nll_cur), p(self.nll_prop), p(self.v_cur), p(self.v_prop), p(self.acc), p(self.cnt), p(self.jb),
                self.P, p(self.jw), p(self.nexpected), p(self.n_mc), p(self.source_id), p(self.norms), 0]

    def step(self, block, total, factor=None, whitening=None, constrained=True):
        if constrained:
            capi.call("sxmc_launch_finish_nll_jump_pick_combo_constrained", *self.args(block, total), capi.ptr(factor),
                      capi.ptr(whitening))
        else:
            capi.call("sxmc_launch_finish_nll_jump_pick_combo", *self.args(block, total))

    def offsets(self):
        return [int(o) for o in self.rngs.get().reshape(self.P, 4)[:, 2]]

    def state(self):
        capi.synchronize()
        return b"".join(a.get().tobytes() for a in (self.v_cur, self.v_prop, self.nll_cur, self.nll_prop, self.acc,
                                                    self.cnt, self.jb, self.rngs))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def signal_term(p0):
    return np.float64(p0) * np.float64(NEXPECTED) * np.float64(NORM) / np.float64(N_MC)


def make(P, fixed, unconstrained):
    rng = np.random.default_rng(3000 + P + 7 * len(fixed) + sum(fixed) + 11 * sum(unconstrained))
    widths = (0.02 + 0.05 * rng.random(P)).astype(np.float32)
    widths[list(fixed)] = -1.0
    means = 50.0 + rng.standard_normal(P)
    sigmas = 0.05 + 0.2 * rng.random(P)
    for n, i in enumerate(unconstrained):
        sigmas[i] = 0.0 if n % 2 == 0 else -1.0
    v0 = means + 0.5 * sigmas.clip(min=0.05) * rng.standard_normal(P)       # (fixed parameters off their means too)
    constrained = np.flatnonzero(sigmas > 0)
    rho = sc.block_matrix(P, [(constrained, sc.random_correlation(constrained.size, rng))]) if constrained.size > 1 \
        else np.eye(P)
    W = nll.constraint_whitening(rho, sigmas).reshape(P, P).T
    L = np.tril(0.05 * rng.standard_normal((P, P)) / np.sqrt(np.arange(1, P + 1))[:, None])
    return widths, means, sigmas, v0, rho, W, L


def on_device(M):
    """A lower-triangular [P, P] matrix in the device's layout, NaN above the diagonal."""
    M = np.array(M, np.float64)
    M[np.triu_indices(M.shape[0], 1)] = np.nan
    return DeviceArray(sc.device_layout(M))


@pytest.mark.parametrize("with_factor", [False, True], ids=["diagonal", "factor"])
@pytest.mark.parametrize("P,fixed,unconstrained,block,nsteps", CASES)
def test_step_end_with_a_dense_whitening_matrix_equals_the_replay_as_bytes(P, fixed, unconstrained, block, nsteps,
                                                                           with_factor):
    widths, means, sigmas, v0, rho, W, L = make(P, fixed, unconstrained)
    free = widths > 0
    d_W = on_device(W)
    d_L = on_device(L) if with_factor else None
    rng = np.random.default_rng(P)
    nll0 = sc.nll_total(-100.0, v0, means, sigmas, 0, (signal_term(v0[0]),), W)
    c = Chain(P, 0, means, sigmas, widths, v0, nll0, nsteps + 1)
    twin = Chain(P, 0, np.zeros(P), np.zeros(P), np.where(free, 1.0, -1.0), np.zeros(P), 0.0, nsteps + 1)
    cls = cov.StepReferenceCov if with_factor else sc.StepReference
    kw = dict(factor=L) if with_factor else {}
    ref = cls(SEED, widths, v0, nll0, c.nrows, fill=FILL, **kw)
    c.first_proposal()
    twin.first_proposal()
    ref.first_proposal()
    capi.synchronize()
    z = twin.v_prop.get()
    assert np.all(np.abs(z - ref.last_z) <= 8e-12) and np.all(z[~free] == 0.0)
    assert np.all(np.abs(c.v_prop.get() - ref.v_proposed) <= 8e-12 * np.abs(widths) + 2.0 ** -52 * np.abs(ref.v_proposed))
    ref.v_proposed = c.v_prop.get()
    accepted = 0
    pen0 = sc.nll_total(0.0, v0, means, sigmas, 0, (), W)
    for k in range(nsteps):
        p = c.v_prop.get()                                   # the vector this step decides on, as the device holds it
        # event sums that make the NLLs of neighbouring steps comparable: most decisions fall to the uniform
        # (the constraints of up to 256 parameters move by far more than that from step to step: the handed-in sum takes
        # their change since the start back out, so that only its own noise is left -- it is an input like any other)
        total = -100.0 + rng.choice([0.3, 1.0, 6.0]) * rng.standard_normal() + \
            (sc.nll_total(0.0, p, means, sigmas, 0, (), W) - pen0)
        want = sc.nll_total(total, p, means, sigmas, 0, (signal_term(p[0]),), W)
        c.step(block, total, d_L, d_W)
        twin.step(block, -1e300, constrained=False)          # NLL 1e300 against 0: refused, the twin stays at 0
        capi.synchronize()
        got = c.nll_prop.get()
        assert bits(got)[0] == bits(np.array([want]))[0], (k, got[0], want)
        rec = ref.step(want)
        accepted += rec["accept"]
        z = twin.v_prop.get()
        assert int(twin.acc.get()[0]) == 0 and np.all(twin.v_cur.get() == 0.0)
        assert np.all(np.abs(z - ref.last_z) <= 8e-12), k
        ref.last_z = z
        ref.v_proposed = cov.propose_cov(z, ref.factor, widths, ref.v_current) if with_factor \
            else sc_propose(z, widths, ref.v_current)
        assert np.array_equal(bits(c.v_prop.get()), bits(ref.v_proposed)), k
        assert np.array_equal(bits(c.v_cur.get()), bits(ref.v_current)), k
        assert bits(c.nll_cur.get())[0] == bits(np.array([ref.nll_current]))[0], k
        assert (int(c.acc.get()[0]), int(c.cnt.get()[0])) == (ref.accepted, ref.count) == (accepted, k + 1)
        assert np.array_equal(bits(c.jb.get().reshape(c.nrows, P + 1)), bits(ref.jump_buffer)), k
        assert c.offsets() == ref.offsets == twin.offsets(), k
    print("P=%d: %d of %d accepted" % (P, accepted, nsteps))
    assert 0 < accepted <= nsteps


def test_planted_wrong_laws_are_told_from_the_device():
    """The comparison above is one of bits, and it must be able to fail: at 17 parameters, with an NLL that is the
    constraints' alone (an expected rate of 0, an event sum of -3.25 -- beside an NLL in the hundreds an ulp of a constraint
    term is lost), twelve vectors are decided on; the device's NLL is the law's bits at every one, and each planted law
    -- W = T, the product descending, one extra term at the end, sigma after the product, no matrix at all -- differs
    from the device at one of them at least."""
    P = 17
    widths, means, sigmas, v0, rho, W, L = make(P, (5, 9), (0, 12))
    d_W = on_device(W)
    rng = np.random.default_rng(5)
    c = Chain(P, 0, means, sigmas, widths, v0, 0.0, 13)
    c.nexpected = DeviceArray(np.zeros(1))
    told = dict.fromkeys(["W = T", "descending", "one extra term", "sigma after the product", "independent"], 0)
    for k in range(12):
        p = means + sigmas.clip(min=0.05) * rng.standard_normal(P)
        c.v_prop.set(p)
        c.step(128, -3.25, None, d_W)
        capi.synchronize()
        got = c.nll_prop.get()
        terms = (np.float64(p[0]) * 0.0,)
        want = sc.nll_total(-3.25, p, means, sigmas, 0, terms, W)
        assert bits(got)[0] == bits(np.array([want]))[0], (k, got[0], want)
        planted = {
            "W = T": sc.nll_total(-3.25, p, means, sigmas, 0, terms, pens=sc.penalties_with_T(p, means, sigmas, rho)),
            "descending": sc.nll_total(-3.25, p, means, sigmas, 0, terms, pens=sc.penalties_descending(p, means, sigmas, W)),
            "one extra term": sc.nll_total_extra_term(-3.25, p, means, sigmas, 0, terms, W),
            "sigma after the product": sc.nll_total(-3.25, p, means, sigmas, 0, terms,
                                                    pens=sc.penalties_sigma_after(p, means, sigmas, W)),
            "independent": sc.nll_total(-3.25, p, means, sigmas, 0, terms)}
        for name, value in planted.items():
            told[name] += int(bits(np.array([value]))[0] != bits(got)[0])
    print("planted laws told at", told, "of 12 vectors")
    assert all(n > 0 for n in told.values()), told


def sc_propose(z, widths, current):
    from tests.step_reference import propose
    return propose(z, widths, current)


@pytest.mark.parametrize("P,fixed,unconstrained,block", [(2, (), (), 64), (17, (5, 9), (0, 12), 128),
                                                         (256, (100,), (255,), 128)])
def test_negative_rate_and_nan_sum_are_1e18_either_way(P, fixed, unconstrained, block):
    widths, means, sigmas, v0, rho, W, L = make(P, fixed, unconstrained)
    d_W = on_device(W)
    nsources = min(P, 3)
    for whitening in (None, d_W):
        for what in ("negative rate", "nan sum", "both", "neither"):
            c = Chain(P, nsources, means, sigmas, widths, v0, 100.0, 2)
            p = v0.copy()
            if what in ("negative rate", "both"):
                p[nsources - 1] = -1e-300            # the last source
            c.v_prop.set(p)
            total = np.nan if what in ("nan sum", "both") else -100.0
            c.step(block, total, None, whitening)
            capi.synchronize()
            got = c.nll_prop.get()[0]
            if what == "neither":
                want = sc.nll_total(total, p, means, sigmas, nsources, (signal_term(p[0]),),
                                    W if whitening is not None else None)
                assert bits(np.array([got]))[0] == bits(np.array([want]))[0] and got != 1e18
            else:
                assert got == 1e18, (what, got)
                assert int(c.acc.get()[0]) == 0 and int(c.cnt.get()[0]) == 1
                assert np.array_equal(bits(c.jb.get()[:P]), bits(v0.astype(np.float32)))


@pytest.mark.parametrize("P,fixed,unconstrained,block", [(1, (), (), 128), (17, (5, 9), (0, 12), 96),
                                                         (256, (100, 101, 200), (0, 255), 128)])
def test_identity_and_null_are_the_existing_launch_point_as_bytes(P, fixed, unconstrained, block):
    widths, means, sigmas, v0, rho, W, L = make(P, fixed, unconstrained)
    d_I = on_device(np.eye(P))
    rng = np.random.default_rng(P)
    noise = rng.choice([0.3, 1.0, 6.0], size=12) * rng.standard_normal(12)
    pen0 = sc.nll_total(0.0, v0, means, sigmas, 0, ())
    nll0 = sc.nll_total(-100.0, v0, means, sigmas, 0, (signal_term(v0[0]),))
    chains = [Chain(P, 0, means, sigmas, widths, v0, nll0, 13) for _ in range(3)]
    for c in chains:
        c.first_proposal()
    for k in range(12):
        # (the sum takes the constraints' change since the start back out, as above: both outcomes of a step occur)
        capi.synchronize()
        total = -100.0 + noise[k] + (sc.nll_total(0.0, chains[0].v_prop.get(), means, sigmas, 0, ()) - pen0)
        chains[0].step(block, total, constrained=False)              # the launch point that was there before
        chains[1].step(block, total, None, None)                     # the new one, both pointers null
        chains[2].step(block, total, None, d_I)                      # W = I
    states = [c.state() for c in chains]
    assert states[0] == states[1] == states[2]
    assert 0 < int(chains[0].acc.get()[0]) <= 12


@pytest.mark.parametrize("P", [257, 300])
def test_a_whitening_matrix_beyond_the_staged_form_is_refused(P):
    widths, means, sigmas, v0, rho, W, L = make(P, (), ())
    c = Chain(P, 0, means, sigmas, widths, v0, 100.0, 2)
    d_W = on_device(np.eye(P))
    c.first_proposal()
    before = c.state()
    with pytest.raises(capi.SxmcError) as e:
        c.step(128, -100.0, None, d_W)
    assert e.value.code == capi.ERR_SHAPE and "256 parameters" in e.value.msg and "whitening" in e.value.msg
    assert c.state() == before                                   # nothing was launched
    c.step(128, -100.0, None, None)                              # without one: the unstaged form, as ever
    capi.synchronize()
    assert int(c.cnt.get()[0]) == 1


@pytest.mark.parametrize("P", [2, 17, 300])
def test_nll_total_whitened_is_the_law_at_any_length(P):
    """The sequential launch point (no staging: any number of parameters), as the reference form's first NLL uses it."""
    widths, means, sigmas, v0, rho, W, L = make(P, (), (1,) if P > 2 else ())
    d_W = on_device(W)
    c = Chain(P, 1, means, sigmas, widths, v0, 0.0, 1)
    out = DeviceArray.zeros(1, np.float64)
    total = DeviceArray(np.array([-12.5]))
    args = [1, 1, capi.ptr(None), P, capi.ptr(c.v_cur), 1, 1, capi.ptr(c.means), capi.ptr(c.sigmas), capi.ptr(total),
            capi.ptr(c.nexpected), capi.ptr(c.n_mc), capi.ptr(c.source_id), capi.ptr(c.norms), capi.ptr(out)]
    capi.call("sxmc_launch_nll_total_whitened", *args, capi.ptr(d_W))
    capi.synchronize()
    want = sc.nll_total(-12.5, v0, means, sigmas, 1, (signal_term(v0[0]),), W)
    assert bits(out.get())[0] == bits(np.array([want]))[0]
    capi.call("sxmc_launch_nll_total_whitened", *args, capi.ptr(None))
    capi.synchronize()
    plain = out.get()[0]
    capi.call("sxmc_launch_nll_total", *args)
    capi.synchronize()
    assert bits(out.get())[0] == bits(np.array([plain]))[0] == bits(np.array([sc.nll_total(
        -12.5, v0, means, sigmas, 1, (signal_term(v0[0]),))]))[0]
    assert plain != want
