"""CPU: the host side of correlated Gaussian constraints.  sxmc_constraint_whitening (the library's entry point) and the
stand-alone program over the same header (tests/cpp/constraint_whitening_host, plain and under ASan + UBSan) against the
numpy restatement of the law in tests/step_reference_constraints.py, bit for bit; every refusal with its message; the
accuracy of 0.5 sum r_i^2 against 0.5 x^T rho^-1 x solved in long double, within twice the bound derived in that file;
and planted wrong laws, each of which the comparisons of this feature's tests tell from the right one.  The walk plan's
fact (tests/cpp/test_constraint_plan) runs here too."""
import os
import struct
import subprocess

import numpy as np
import pytest

from sxmc_amd import capi, nll
from tests import step_reference_constraints as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def programs():
    names = ["constraint_whitening_host", "constraint_whitening_host_asan", "test_constraint_plan",
             "test_constraint_plan_asan"]
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "constraints.mk"] + names)
    return {n: os.path.join(CPP, n) for n in names}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def interleaved():
    """P = 12: blocks {1, 4, 9} and {2, 7} and {10, 11} interleaved with unconstrained (0, 5) and lone (3, 6, 8)
    parameters; 6 and 9 are 'fixed' (nothing in the whitening knows: a fixed parameter may take part)."""
    rng = np.random.default_rng(5)
    b3 = sc.random_correlation(3, rng, 0.9)
    rho = sc.block_matrix(12, [((1, 4, 9), b3), ((2, 7), [[1, 0.8], [0.8, 1]]), ((10, 11), [[1, -0.95], [-0.95, 1]])])
    sigmas = np.array([0, .1, .2, .3, .4, 0, .5, .6, .7, .8, .9, 1.0])
    return rho, sigmas


def near_singular(P, r=0.999):
    """Every pair correlated at r (eigenvalues 1 - r and 1 + (P - 1) r), odd pairs at -r in a 2 x 2 corner."""
    rho = np.full((P, P), r)
    np.fill_diagonal(rho, 1.0)
    return rho


def cases():
    rng = np.random.default_rng(20250101)
    out = {}
    for P in (1, 2, 17, 255, 256):
        out["dense P=%d" % P] = (sc.random_correlation(P, rng), np.full(P, 0.5))
        out["identity P=%d" % P] = (np.eye(P), np.zeros(P))
    out["pair -0.6"] = (np.array([[1.0, -0.6], [-0.6, 1.0]]), np.array([1.0, 2.0]))
    out["interleaved blocks"] = interleaved()
    out["|rho| = 0.999, pair"] = (np.array([[1.0, -0.999], [-0.999, 1.0]]), np.ones(2))
    out["|rho| = 0.999, P=5"] = (near_singular(5), np.ones(5))
    return out


CASES = cases()


def run_host(program, tmp_path, rho, sigmas):
    P = sigmas.size
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("q", P))
        f.write(np.ascontiguousarray(sigmas, np.float64).tobytes())
        f.write(np.ascontiguousarray(rho, np.float64).tobytes())
    r = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(dst, "rb").read()
    status, pivot = struct.unpack("qq", raw[:16])
    if status != 0:
        return status, pivot, None, raw[16:].decode()
    W = np.frombuffer(raw[16:16 + 8 * P * P], np.float64)
    return status, pivot, W, raw[16 + 8 * P * P:].decode()


@pytest.mark.parametrize("name", sorted(CASES))
def test_whitening_matches_the_restatement_bit_for_bit(name, programs, tmp_path):
    rho, sigmas = CASES[name]
    P = sigmas.size
    want = sc.device_layout(sc.whitening(rho))
    got = nll.constraint_whitening(rho, sigmas)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:4]
    for prog in ("constraint_whitening_host", "constraint_whitening_host_asan"):
        status, pivot, W, msg = run_host(programs[prog], tmp_path, rho, sigmas)
        assert (status, pivot, msg) == (0, -1, "")
        assert np.array_equal(bits(W), bits(want)), prog
    W = want.reshape(P, P).T
    assert np.all(W[np.triu_indices(P, 1)] == 0.0) and not np.any(np.signbit(W[np.triu_indices(P, 1)]))
    assert np.all(np.diag(W) > 0)
    if name.startswith("identity"):
        assert np.array_equal(bits(W), bits(np.eye(P)))
    if name == "pair -0.6":
        assert np.array_equal(bits(W), bits(np.array([[1.0, 0.0], [0.75, 1.25]])))
    if name == "interleaved blocks":
        # outside every group: W_ii = 1 and +0 beside it; inside a block: the bytes the block gives alone
        for i in (0, 3, 5, 6, 8):
            row = np.zeros(P)
            row[i] = 1.0
            assert np.array_equal(bits(W[i]), bits(row)), i
        for idx in ((1, 4, 9), (2, 7), (10, 11)):
            idx = np.array(idx)
            alone = sc.whitening(rho[np.ix_(idx, idx)])
            assert np.array_equal(bits(W[np.ix_(idx, idx)]), bits(alone)), idx
            assert np.array_equal(bits(nll.constraint_whitening(rho[np.ix_(idx, idx)], sigmas[idx])),
                                  bits(sc.device_layout(alone)))


def refused(rho, sigmas):
    with pytest.raises(capi.SxmcError) as e:
        nll.constraint_whitening(np.array(rho, np.float64), np.array(sigmas, np.float64))
    assert e.value.code == capi.ERR_INVALID
    return e.value.msg


def test_every_refusal_names_its_entry(programs, tmp_path):
    rho = sc.random_correlation(6, np.random.default_rng(3))
    sig = np.ones(6)

    def with_entry(i, j, v, both=True):
        r = rho.copy()
        r[i, j] = v
        if both:
            r[j, i] = v
        return r

    assert "not symmetric at (4, 2)" in refused(with_entry(4, 2, np.nextafter(rho[4, 2], 1.0), both=False), sig)
    assert "diagonal entry (3, 3) is not 1" in refused(with_entry(3, 3, np.nextafter(1.0, 0.0)), sig)
    assert "entry (1, 5) is not a finite number in [-1, 1]" in refused(with_entry(1, 5, np.nextafter(1.0, 2.0)), sig)
    assert "entry (0, 2) is not a finite number in [-1, 1]" in refused(with_entry(0, 2, np.nan), sig)
    assert "entry (2, 3) is not a finite number in [-1, 1]" in refused(with_entry(2, 3, -np.inf), sig)
    s0 = sig.copy()
    s0[4] = 0.0
    msg = refused(rho, s0)
    assert "parameter 4 has no constraint" in msg and "entry (4, 0) is not 0" in msg
    s0[4] = -1.0
    assert "parameter 4 has no constraint" in refused(rho, s0)
    # the same answers from the restatement, and from the stand-alone program under the sanitizers
    assert sc.refusal(with_entry(4, 2, 0.123, both=False), sig) == ("symmetry", 4, 2)
    assert sc.refusal(with_entry(3, 3, 0.5), sig) == ("diagonal", 3, 3)
    assert sc.refusal(with_entry(1, 5, 1.5), sig) == ("range", 1, 5)
    assert sc.refusal(rho, s0) == ("unconstrained", 4, 0)
    assert sc.refusal(rho, sig) is None
    status, _, W, msg = run_host(programs["constraint_whitening_host_asan"], tmp_path, with_entry(1, 5, 1.5), sig)
    assert status == 1 and W is None and "entry (1, 5)" in msg
    # an unconstrained parameter with zeros beside it is accepted, and stays outside
    r = rho.copy()
    r[4, :] = r[:, 4] = 0.0
    r[4, 4] = 1.0
    s0[4] = 0.0
    W = nll.constraint_whitening(r, s0).reshape(6, 6).T
    assert np.array_equal(bits(W[4]), bits(np.eye(6)[4])) and np.all(W[:, 4] == np.eye(6)[:, 4])


def test_not_positive_definite_names_the_pivot(programs, tmp_path):
    assert "not positive definite at parameter 1" in refused([[1, 1], [1, 1]], [1, 1])
    assert "not positive definite at parameter 1" in refused([[1, -1], [-1, 1]], [1, 1])
    bad = np.array([[1, .9, -.9], [.9, 1, .9], [-.9, .9, 1]])
    assert "not positive definite at parameter 2" in refused(bad, [1, 1, 1])
    with pytest.raises(ValueError, match="parameter 2"):
        sc.whitening(bad)
    # embedded: the pivot is named in the full vector's numbering
    big = sc.block_matrix(9, [((2, 5, 7), bad)])
    assert "not positive definite at parameter 7" in refused(big, np.ones(9))
    status, pivot, W, msg = run_host(programs["constraint_whitening_host_asan"], tmp_path, big, np.ones(9))
    assert (status, pivot, W) == (2, 7, None) and msg.endswith("at parameter 7")


def test_bad_arguments_are_refused():
    lib = capi.load()
    one = np.ones(1)
    assert lib.sxmc_constraint_whitening(None, capi.ptr(one), 1, capi.ptr(one)) == capi.ERR_INVALID
    assert lib.sxmc_constraint_whitening(capi.ptr(one), capi.ptr(one), 0, capi.ptr(one)) == capi.ERR_INVALID
    with pytest.raises(ValueError, match="2 x 2"):
        nll.constraint_whitening(np.eye(3), np.ones(2))


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("name", sorted(CASES))
def test_quadratic_form_within_twice_the_derived_bound(name):
    rho, sigmas = CASES[name]
    P = sigmas.size
    rng = np.random.default_rng(P + 17)
    W = nll.constraint_whitening(rho, np.ones(P)).reshape(P, P).T
    bound = sc.accuracy_bound(rho)
    worst = 0.0
    for trial in range(3):
        x = rng.standard_normal(P) * 10.0 ** rng.integers(-3, 4)
        r = sc.whitened(W, x)
        q = np.float64(0.0)
        for v in 0.5 * r * r:
            q = q + v
        exact = sc.quadratic_form_longdouble(rho, x)
        rel = float(abs(np.longdouble(q) - exact) / exact)
        worst = max(worst, rel)
        assert rel <= 2.0 * bound, (name, trial, rel, bound)
    print("%s: relative error %.3g, bound %.3g, share %.3g" % (name, worst, bound, worst / bound))


# ------------------------------------------------------------------------------------------------ planted wrong laws
def planted_inputs():
    """The step-end test's kind of input: different sigmas, a dense matrix, residuals of order one."""
    rng = np.random.default_rng(77)
    P = 17
    rho = sc.random_correlation(P, rng)
    sigmas = 0.05 + rng.random(P)
    means = rng.standard_normal(P)
    p = means + sigmas * rng.standard_normal(P)
    return rho, sigmas, means, p


def test_planted_wrong_laws_are_each_rejected():
    """What the device tests compare is the NLL's bits at every step (and through the decisions every later row).  A law
    that is the same model in another order of operations can agree in a given NLL's bits by chance, so each planted law
    is run over the twelve vectors of a short walk, as a step-end test does, and must be told at one of them at least."""
    rho, sigmas, means, _ = planted_inputs()
    rng = np.random.default_rng(78)
    W = sc.whitening(rho)
    bound = sc.accuracy_bound(rho)
    told = dict.fromkeys(["W = T", "descending", "one extra term", "sigma after the product"], 0)
    outside = dict.fromkeys(told, 0)
    for trial in range(12):
        p = means + sigmas * rng.standard_normal(sigmas.size)
        right = sc.nll_total(-3.25, p, means, sigmas, 0, (1.5,), W)
        exact = float(sc.quadratic_form_longdouble(rho, sc.residuals(p, means, sigmas)))
        base = 3.25 + 1.5
        slack = 8 * 2.0 ** -53 * abs(right)          # the additions of nll_total itself
        assert abs((right - base) - exact) <= 2.0 * bound * exact + slack
        wrong = {
            "W = T": sc.nll_total(-3.25, p, means, sigmas, 0, (1.5,), pens=sc.penalties_with_T(p, means, sigmas, rho)),
            "descending": sc.nll_total(-3.25, p, means, sigmas, 0, (1.5,),
                                       pens=sc.penalties_descending(p, means, sigmas, W)),
            "one extra term": sc.nll_total_extra_term(-3.25, p, means, sigmas, 0, (1.5,), W),
            "sigma after the product": sc.nll_total(-3.25, p, means, sigmas, 0, (1.5,),
                                                    pens=sc.penalties_sigma_after(p, means, sigmas, W)),
        }
        for name, value in wrong.items():
            told[name] += int(bits(np.array([value]))[0] != bits(np.array([right]))[0])
            outside[name] += int(abs((value - base) - exact) > 2.0 * bound * exact + slack)
    print(told, outside)
    assert all(n > 0 for n in told.values()), told
    # the two that are another model are told by the accuracy bound as well, at every vector; the two that are the same
    # model in another order never are: only a comparison of bits tells them
    assert outside["W = T"] == 12 and outside["sigma after the product"] == 12
    assert outside["descending"] == 0 and outside["one extra term"] == 0


def test_identity_and_blocks_are_exact():
    rho, sigmas, means, p = planted_inputs()
    P = sigmas.size
    sigmas[[2, 9]] = 0.0
    plain = sc.penalties(p, means, sigmas, None)
    assert np.array_equal(bits(sc.penalties(p, means, sigmas, np.eye(P))), bits(plain))
    assert np.signbit(plain[2]) and plain[2] == 0.0
    for total in (-3.25, np.nan):
        assert sc.nll_total(total, p, means, sigmas, 0, (1.5,), np.eye(P)) == sc.nll_total(total, p, means, sigmas, 0, (1.5,))
    neg = p.copy()
    neg[1] = -0.5
    assert sc.nll_total(-3.25, neg, means, sigmas, 3, (1.5,), np.eye(P)) == 1e18
    # a block-diagonal matrix gives inside each block the penalties that block gives alone
    blocks = [np.array([0, 5, 11]), np.array([3, 4])]
    full = sc.block_matrix(P, [(b, rho[np.ix_(b, b)]) for b in blocks])
    pens = sc.penalties(p, means, sigmas, sc.whitening(full))
    for b in blocks:
        alone = sc.penalties(p[b], means[b], sigmas[b], sc.whitening(rho[np.ix_(b, b)]))
        assert np.array_equal(bits(pens[b]), bits(alone))
    rest = np.setdiff1d(np.arange(P), np.concatenate(blocks))
    assert np.array_equal(bits(pens[rest]), bits(plain[rest]))


def test_walk_plan_never_takes_lookahead_or_lockstep(programs):
    for prog in ("test_constraint_plan", "test_constraint_plan_asan"):
        r = subprocess.run([programs[prog]], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "0 failed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
