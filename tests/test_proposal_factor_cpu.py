"""CPU: sxmc_proposal_factor, the one implementation of a correlated proposal's re-tuning (include/sxmc_hip.h), against
the replay's (tests/step_reference_cov.py) bit for bit; the algebra of what it returns; the same code as a stand-alone
program under ASan + UBSan on the same cases; the replay's own fma against exact rational arithmetic."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from sxmc_amd import capi, nll
from tests import step_reference_cov as cov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "cpp", "proposal_factor_host")


def chain_rows(rng, n, P, mix=0.6):
    """n correlated rows of P parameters and an NLL column, as a jump buffer holds them."""
    base = rng.standard_normal((n, P))
    common = rng.standard_normal((n, 1))
    x = (1.0 + 0.1 * np.arange(P)) * (base + mix * common) + 3.0
    return np.concatenate([x, rng.standard_normal((n, 1))], axis=1).astype(np.float32)


def widths(rng, P, fixed=()):
    w = (0.05 + rng.random(P)).astype(np.float32)
    w[list(fixed)] = -1.0
    return w


def make_cases():
    rng = np.random.default_rng(20240611)
    c = {}
    c["no_rows"] = (np.zeros((0, 6), np.float32), widths(rng, 5), 0.05)
    c["one_row"] = (chain_rows(rng, 1, 4), widths(rng, 4), 0.05)
    c["P1"] = (chain_rows(rng, 50, 1), widths(rng, 1), 0.05)
    c["P256"] = (chain_rows(rng, 300, 256), widths(rng, 256, fixed=(7, 100)), 0.05)
    r = chain_rows(rng, 80, 5)
    r[:, 2] = np.float32(1.25)
    c["zero_spread_column"] = (r, widths(rng, 5), 0.05)
    c["fixed_first"] = (chain_rows(rng, 60, 6), widths(rng, 6, fixed=(0,)), 0.05)
    c["fixed_last"] = (chain_rows(rng, 60, 6), widths(rng, 6, fixed=(5,)), 0.05)
    c["fixed_interleaved"] = (chain_rows(rng, 60, 7), widths(rng, 7, fixed=(1, 3, 4)), 0.2)
    r = chain_rows(rng, 90, 5)
    r[:, 3] = r[:, 1]
    c["identical_columns"] = (r, widths(rng, 5), 0.05)
    # the same singular R with a shrinkage too small to be seen beside 1: (1 - b) rounds to 1, the second of the two
    # identical columns meets the pivot 1 - 1 = 0, and b doubles until 1 - b < 1
    c["pivot_fails_shrinkage_doubles"] = (r.copy(), widths(rng, 5), 2.0 ** -60)
    # the cap: at shrinkage 1 nothing is factored, T = I
    c["shrinkage_one_is_identity"] = (chain_rows(rng, 40, 3), widths(rng, 3), 1.0)
    # a column that holds an infinity has no spread to speak of (its sums are not numbers): decoupled like a constant one
    r = chain_rows(rng, 40, 4)
    r[5, 1] = np.inf
    c["infinite_column_decouples"] = (r, widths(rng, 4), 0.05)
    return c


CASES = make_cases()
_REPLAY = {}


def replay(name):
    if name not in _REPLAY:
        rows, w, b = CASES[name]
        with np.errstate(all="ignore"):
            _REPLAY[name] = cov.retune_factor(rows, w, b)
    return _REPLAY[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_equals_the_replay_bit_for_bit(name):
    rows, w, b = CASES[name]
    L, _, _, used = replay(name)
    got, got_used = nll.proposal_factor(rows, w, b)
    print("%s: shrinkage %r -> used %r" % (name, b, got_used))
    assert got_used == used
    assert got.tobytes() == cov.device_layout(L).tobytes()


def test_expected_shrinkages():
    assert replay("identical_columns")[3] == 0.05                 # R singular: the default suffices
    assert replay("no_rows")[3] == 0.05
    used = replay("pivot_fails_shrinkage_doubles")[3]
    print("pivot_fails_shrinkage_doubles: shrinkage_used = %r" % used)
    assert 2.0 ** -60 < used < 1e-15 and used == 2.0 ** round(np.log2(used))    # doubled, a power of two still
    assert replay("shrinkage_one_is_identity")[3] == 1.0
    rows, w, _ = CASES["shrinkage_one_is_identity"]
    assert np.array_equal(replay("shrinkage_one_is_identity")[0], np.diag(w.astype(np.float64)))
    L = replay("infinite_column_decouples")[0]
    assert L[1, 0] == 0.0 and np.all(L[2:, 1] == 0.0) and L[2, 0] != 0.0


def test_no_rows_is_the_diagonal_proposal():
    rows, w, b = CASES["no_rows"]
    got, _ = nll.proposal_factor(rows, w, b)
    assert got.tobytes() == cov.device_layout(cov.diagonal_factor(w)).tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_factor_algebra(name):
    """L L^T = W R_b W to 1e-12 relative (of w_i w_j: R_b's entries are at most 1), T's rows have norm 1 to 1e-14,
    fixed parameters' rows and columns are zero, nothing stands above the diagonal."""
    rows, w, b = CASES[name]
    P = w.size
    _, _, A, _ = replay(name)
    got, _ = nll.proposal_factor(rows, w, b)
    L = got.reshape(P, P).T
    free = w > 0
    wd = np.where(free, w.astype(np.float64), 0.0)
    assert np.all(L[~free, :] == 0.0) and np.all(L[:, ~free] == 0.0) and np.all(np.triu(L, 1) == 0.0)
    want = wd[:, None] * np.where(free[:, None] & free[None, :], A, 0.0) * wd[None, :]
    err = np.abs(L @ L.T - want)
    scale = np.outer(wd, wd)
    worst = float(np.max(err[scale > 0] / scale[scale > 0])) if np.any(scale > 0) else 0.0
    T = L[free] / wd[free, None]
    norms = np.sum(T * T, axis=1)
    print("%s: max |L L^T - W R_b W| / (w_i w_j) = %.3g, max |row norm - 1| = %.3g"
          % (name, worst, float(np.max(np.abs(norms - 1.0)))))
    assert worst <= 1e-12
    assert np.all(np.abs(norms - 1.0) <= 1e-14)


def test_marginal_widths_are_the_reference_s():
    """Every parameter's marginal proposal width is w_i: the variance of (L z)_i is sum_j L_ij^2 = w_i^2."""
    rows, w, b = CASES["identical_columns"]
    L = nll.proposal_factor(rows, w, b)[0].reshape(w.size, w.size).T
    assert np.allclose(np.sqrt(np.sum(L * L, axis=1)), w.astype(np.float64), rtol=1e-14, atol=0)


def test_refusals_need_no_device():
    w = np.ones(2, np.float32)
    rows = np.zeros((3, 3), np.float32)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(capi.SxmcError) as e:
            nll.proposal_factor(rows, w, bad)
        assert e.value.code == capi.ERR_INVALID and "(0, 1]" in e.value.msg
    out = np.zeros(4)
    lib = capi.load()
    assert lib.sxmc_proposal_factor(None, 3, 2, capi.ptr(w), 0.05, capi.ptr(out), None) == capi.ERR_INVALID
    assert lib.sxmc_proposal_factor(capi.ptr(rows), 3, 0, capi.ptr(w), 0.05, capi.ptr(out), None) == capi.ERR_INVALID
    assert lib.sxmc_proposal_factor(capi.ptr(rows), 3, 2, None, 0.05, capi.ptr(out), None) == capi.ERR_INVALID
    assert lib.sxmc_proposal_factor(capi.ptr(rows), 3, 2, capi.ptr(w), 0.05, None, None) == capi.ERR_INVALID
    assert lib.sxmc_proposal_factor(capi.ptr(rows), 3, 2, capi.ptr(w), 0.05, capi.ptr(out), None) == capi.OK


@pytest.mark.parametrize("program", ["proposal_factor_host", "proposal_factor_host_asan"])
def test_stand_alone_program_equals_the_replay(program, tmp_path):
    """The same code with its own main, plain and built with -fsanitize=address,undefined: every case, bit for bit, and
    not a word from either sanitizer."""
    exe = os.path.join(ROOT, "tests", "cpp", program)
    assert os.path.exists(exe), "__graft_entry__.build() builds tests/cpp/%s (proposal.mk)" % program
    for name in sorted(CASES):
        rows, w, b = CASES[name]
        src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
        src.write_bytes(struct.pack("=qqd", w.size, rows.shape[0], b) + w.tobytes() + np.ascontiguousarray(rows).tobytes())
        p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", (name, p.returncode, p.stderr[-2000:])
        out = np.frombuffer(dst.read_bytes(), np.float64)
        L, _, _, used = replay(name)
        assert out[0] == used, name
        assert out[1:].tobytes() == cov.device_layout(L).tobytes(), name


def test_replay_fma_is_the_exact_value_rounded_once():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a, b = rng.standard_normal(2) * 10.0 ** rng.integers(-8, 8)
        c = -a * b * (1.0 + rng.standard_normal() * 2.0 ** -rng.integers(20, 54)) if rng.random() < 0.5 \
            else float(rng.standard_normal())
        a, b, c = float(a), float(b), float(c)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        if exact != 0:
            assert cov.fma(a, b, c) == float(exact)
    assert cov.fma(0.0, 5.0, 0.0) == 0.0 and cov.fma(2.0, 3.0, -6.0) == 0.0


def test_replay_proposal_orders_its_terms():
    """d_i takes its terms in ascending j, one rounding per term: against exact arithmetic rounded after every term."""
    rng = np.random.default_rng(9)
    P = 9
    L = np.tril(rng.standard_normal((P, P)))
    z = rng.standard_normal(P)
    cur = rng.standard_normal(P) * 100.0
    jw = np.ones(P, np.float32)
    jw[4] = -1.0
    got = cov.propose_cov(z, L, jw, cur)
    for i in range(P):
        if i == 4:
            assert got[i] == cur[i]
            continue
        d = 0.0
        for j in range(i + 1):
            d = float(Fraction(float(L[i, j])) * Fraction(float(z[j])) + Fraction(d))
        assert got[i] == cur[i] + d
