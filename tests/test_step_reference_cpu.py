"""CPU: the host replay of the step end (tests/step_reference.py) against the C oracle's jump_decider / pick_new_vector,
its random law against hand values and the Random123 known answers, and -- this is where the seeds are chosen -- the
conditions every case of tests/test_gpu_step_replay.py relies on, asserted on the reference alone:

  every ordinary case refuses at least 20 of its steps and accepts at least 20 uphill ones, so that a decision rule
  that is wrong either way, a wrong uniform or a wrong row after a rejection cannot go unseen;
  no uphill decision is closer than 1e-4 (relative, of exp(nc - np)) to its uniform: the 1e-12 the device's NLL may
  differ from the oracle's moves exp(nc - np) by 1e-12 * |NLL| < 1e-7, never a decision.

Figures (python -m tests.step_replay_cases prints them): README, "Reproducing the numbers".
"""
import math

import numpy as np
import pytest

from oracle import oracle
from tests import step_reference as sr
from tests import step_replay_cases as cases
from tests.helpers import philox4x32_10


def test_word_maps_at_their_ends():
    assert sr.word_to_uniform(0) == 2.0 ** -32 and sr.word_to_uniform(2 ** 32 - 1) == 1.0      # (0, 1]
    assert sr.word_to_uniform(2 ** 31 - 1) == 0.5
    # normal: the radius from word 0 (largest at word 0, zero at 2^32 - 1), the angle from word 1 in [0, 2 pi)
    r0 = math.sqrt(64.0 * math.log(2.0))                     # sqrt(-2 ln 2^-32) = 6.6604...
    assert sr.words_to_normal(0, 0) == pytest.approx(r0, rel=1e-15) and r0 < 6.7
    assert sr.words_to_normal(2 ** 32 - 1, 0) == 0.0 and sr.words_to_normal(2 ** 32 - 1, 2 ** 32 - 1) == 0.0
    assert sr.words_to_normal(0, 2 ** 31) == pytest.approx(-r0, rel=1e-15)                     # angle pi
    assert abs(sr.words_to_normal(0, 2 ** 30)) < 1e-14                                         # angle pi / 2
    assert sr.words_to_normal(0, 2 ** 32 - 1) == pytest.approx(r0 * math.cos(2 * math.pi * (1 - 2.0 ** -32)), rel=1e-15)
    u1 = (12345 + 1) * 2.0 ** -32
    assert sr.words_to_normal(12345, 2 ** 29) == math.sqrt(-2.0 * math.log(u1)) * math.cos(
        6.283185307179586 * 0.125)


def test_random123_known_answers_through_the_counter_layout():
    """The vectors of test_philox_known_answers_and_stream_layout (tests/test_gpu_nll.py): counter words (offset low,
    offset high, index low, index high), key words (seed low, seed high)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        seed, offset, index = key[0] | (key[1] << 32), ctr[0] | (ctr[1] << 32), ctr[2] | (ctr[3] << 32)
        assert sr.generator_words(seed, index, offset) == want == philox4x32_10(ctr, key)
    # a StepReference draws through the same layout and advances the offset by one per draw, carrying into the high word
    ref = sr.StepReference(0xa4093822 | (0x299f31d0 << 32), [1.0, -1.0, 1.0], np.zeros(3), 0.0, 1,
                           offsets=[2 ** 32 - 1, 5, 2 ** 32 - 1])
    w = philox4x32_10((0xffffffff, 0, 0, 0), (0xa4093822, 0x299f31d0))
    assert ref.draw_uniform() == (w[0] + 1) * 2.0 ** -32 and ref.offsets == [2 ** 32, 5, 2 ** 32 - 1]
    z = ref.draw_normals()
    w0 = philox4x32_10((0, 1, 0, 0), (0xa4093822, 0x299f31d0))
    w2 = philox4x32_10((0xffffffff, 0, 2, 0), (0xa4093822, 0x299f31d0))
    assert z[0] == sr.words_to_normal(w0[0], w0[1]) and z[1] == 0.0 and z[2] == sr.words_to_normal(w2[0], w2[1])
    assert ref.offsets == [2 ** 32 + 1, 5, 2 ** 32]           # (the fixed parameter's generator is not drawn from)


def test_the_uniform_that_is_exactly_one():
    assert sr.generator_words(1, 0, cases.ONE_AT_OFFSET)[0] == 0xFFFFFFFF
    assert sr.word_to_uniform(sr.generator_words(1, 0, cases.ONE_AT_OFFSET)[0]) == 1.0
    c = cases.CASE["uniform_is_1"]
    assert c.seed == 1 and c.offsets0()[0] + cases.ONE_AT_STEP == cases.ONE_AT_OFFSET and not np.any(
        c.tables()["jump_width"] > 0)


def test_order_of_draws():
    """Set-up: one normal per free parameter.  A step: generator 0's uniform FIRST -- also with parameter 0 fixed --
    then one normal per free parameter."""
    seed = 77
    for jw in ([0.5, 0.25, -1.0], [-1.0, 0.25, 0.5], [-1.0, -1.0, -1.0]):
        free = [w > 0 for w in jw]
        ref = sr.StepReference(seed, jw, [1.0, 2.0, 3.0], 10.0, 4)
        ref.first_proposal()
        assert ref.offsets == [int(f) for f in free]
        for i in range(3):
            w = sr.generator_words(seed, i, 0)
            want = [1.0, 2.0, 3.0][i] + float(np.float32(jw[i])) * sr.words_to_normal(w[0], w[1]) if free[i] else \
                [1.0, 2.0, 3.0][i]
            assert ref.v_proposed[i] == want
        rec = ref.step(10.5)
        assert rec["u"] == sr.word_to_uniform(sr.generator_words(seed, 0, int(free[0]))[0])
        assert ref.offsets == [1 + 2 * int(free[0]), 2 * int(free[1]), 2 * int(free[2])]
        w = sr.generator_words(seed, 0, 2)
        if free[0]:
            assert ref.last_z[0] == sr.words_to_normal(w[0], w[1])


def test_transition_is_the_c_oracles_bit_for_bit():
    """Given the same u and z: oracle.jump_decider + oracle.pick_new_vector (nll_kernels.cpp:30-86 in C)."""
    rng = np.random.default_rng(8)
    P, nrows = 7, 64
    jw = rng.uniform(0.01, 0.5, P).astype(np.float32)
    jw[2] = -1.0

    def follow(nll0, special, nsteps):
        ref = sr.StepReference(5, jw, rng.normal(size=P), nll0, nrows, accepted=2, count=3, fill=-7.5)
        ref.first_proposal()
        o_cur, o_nc = ref.v_current.copy(), np.array([nll0])
        o_acc, o_cnt = np.array([2], np.int32), np.array([3], np.int32)
        o_buf = np.full(nrows * (P + 1), -7.5, np.float32)
        o_prop = oracle.pick_new_vector(ref.last_z, jw, o_cur)
        assert np.array_equal(o_prop, ref.v_proposed)
        for k in range(nsteps):
            np_ = special[k] if k < len(special) else float(ref.nll_current + rng.normal(0.0, 1.5))
            rec = ref.step(np_)
            with np.errstate(over="ignore"):
                oracle.jump_decider(rec["u"], o_nc, np.array([np_]), o_cur, o_prop, o_acc, o_cnt, o_buf)
            assert ref.accepted == o_acc[0] and ref.count == o_cnt[0] == 4 + k
            assert np.array_equal(ref.v_current, o_cur)
            assert ref.nll_current == o_nc[0]
            assert np.array_equal(ref.jump_buffer.ravel().view(np.uint32), o_buf.view(np.uint32))
            o_prop = oracle.pick_new_vector(ref.last_z, jw, o_cur)
            assert np.array_equal(o_prop, ref.v_proposed)
        return ref

    # 1e18 -> 1e18 is a tie (accepted); +inf or 1e18 from a finite value, and NaN, are refused
    ref = follow(1e18, [1e18, math.inf, 50.0, 1e18, math.inf, math.nan, 50.0, 2.0], nrows - 3)
    assert [r["accept"] for r in ref.decisions[:8]] == [True, False, True, False, False, False, True, True]
    assert 10 < ref.accepted - 2 < nrows - 13
    assert np.all(ref.jump_buffer[:3] == -7.5) and not np.any(ref.jump_buffer[3:] == -7.5)
    # inf - inf is refused both ways; a finite proposal from +inf is accepted
    ref = follow(math.inf, [math.inf, math.nan, 7.0, -math.inf, -math.inf, 0.0], 6)
    assert [r["accept"] for r in ref.decisions] == [False, False, True, True, False, False]
    # the decision's corners: ties accept (exp(0) = 1 >= every u), inf - inf does not, '<=' holds at equality
    assert sr.decide(1.0, 1e18, 1e18) and not sr.decide(0.5, math.inf, math.inf) and sr.decide(0.9, math.inf, 1.0)
    assert sr.decide(math.exp(-1.0), 0.0, 1.0) and not sr.decide(math.nextafter(math.exp(-1.0), 1.0), 0.0, 1.0)
    assert not sr.decide(2.0 ** -32, 0.0, 1e18) and sr.decide(0.999, 5.0, 4.0) and sr.decide(1.0, 0.0, 800.0, True)
    assert sr.margin_of(0.5, 5.0, 4.0) is None and sr.margin_of(0.5, 0.0, 1e18) == math.inf
    assert sr.margin_of(0.5, 1.0, 1.0) == 0.5 and sr.margin_of(0.5, math.inf, math.inf) == math.inf


def test_retune_and_walk_bookkeeping():
    """mcmc.cpp:274-311 on a made-up NLL: widths from the kept rows' spread (old width where it is 0) times
    (float)(2.4^2 / nfloat), rows dropped at both re-tunings, the proposal drawn before a re-tuning kept."""
    jw0 = np.array([0.3, -1.0, 0.2, 0.1], np.float32)

    def nll_of(v):
        return 0.5 * float(np.sum((np.asarray(v) / [1.0, 1.0, 0.5, 0.3]) ** 2))

    rows, accepted, ref, steps = sr.replay_walk(nll_of, 3, [0.0, 1.0, 0.0, 0.0], jw0, 50, 0.2)
    assert rows.shape == (30, 5) and list(steps) == list(range(20, 50)) and ref.count == 50
    assert accepted == sum(r["accept"] for r in ref.decisions) and 5 < accepted < 45
    assert np.all(rows[:, 1] == 1.0)
    # the same walk by hand up to the first re-tuning
    again = sr.StepReference(3, jw0, [0.0, 1.0, 0.0, 0.0], nll_of([0.0, 1.0, 0.0, 0.0]), 50)
    again.first_proposal()
    for _ in range(10):
        again.step(nll_of(again.v_proposed))
    drawn_before = again.v_proposed.copy()
    kept = again.jump_buffer[:10].copy()
    kept[:, 3] = 0.25                                         # (a free parameter that has not moved: its width stays)
    again.retune(kept)
    kept = kept.astype(np.float64)
    scale = float(np.float32(2.4 * 2.4 / 3))
    assert again.jump_width[0] == np.float32(scale * kept[:, 0].std()) and again.jump_width[1] == -1.0
    assert again.jump_width[2] == np.float32(scale * kept[:, 2].std())
    assert kept[:, 3].std() == 0.0 and again.jump_width[3] == np.float32(scale * float(np.float32(0.1)))
    assert np.array_equal(again.v_proposed, drawn_before)
    # debug mode keeps every row and accepts every step
    rows, accepted, ref, steps = sr.replay_walk(nll_of, 3, [0.0, 1.0, 0.0, 0.0], jw0, 50, 0.2, debug_mode=True)
    assert rows.shape == (50, 5) and accepted == 50


@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_conditions_of_the_launch_point_cases(case):
    ref = case.replay_alone()
    s = cases.check_conditions(case, ref)
    print(case.name, "seed", case.seed, "accepted fraction %.3f" % (s["accepted"] / s["steps"]),
          "smallest margin %.3g" % s["min_margin"])
    t = case.tables()
    free = t["jump_width"] > 0
    assert ref.count == case.count0 + cases.NSTEPS
    assert ref.offsets[0] == case.offsets0()[0] + cases.NSTEPS + (cases.NSTEPS + 1) * int(free[0])
    for i in range(1, case.P):
        assert ref.offsets[i] == case.offsets0()[i] + (cases.NSTEPS + 1) * int(free[i])
    assert np.all(ref.jump_buffer[: case.count0] == 0.0) and np.all(ref.jump_buffer[ref.count:] == 0.0)
    if case.name == "counters_above_0":
        assert case.offset0 < 2 ** 32 < ref.offsets[0]                  # the offset's carry is in the run
    assert case.nsources < case.P or case.P == 1


@pytest.mark.parametrize("name,seed", [(n, s) for n, seeds in cases.WALKS.items() for s in seeds])
def test_conditions_of_the_walks(name, seed):
    rows, accepted, ref, steps = cases.replayed_walk(name, seed)
    s = cases.check_walk_conditions(name, seed, ref)
    print(name, "seed", seed, "accepted fraction %.3f" % (s["accepted"] / s["steps"]),
          "smallest margin %.3g" % s["min_margin"])
    burnin = int(cases.WALK_STEPS * cases.WALK_BURNIN)
    assert rows.shape[0] == cases.WALK_STEPS - 2 * burnin and steps[0] == 2 * burnin
    w = cases.workload_cached(name)
    assert rows.shape[1] == w.nparameters + 1 and np.all(np.isfinite(rows))
    # both re-tunings changed the widths, and rejections repeat rows among those kept
    assert np.any(np.all(rows[1:] == rows[:-1], axis=1))
