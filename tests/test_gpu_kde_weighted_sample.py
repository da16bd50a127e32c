"""The event sampler of a pdfz::EvalKernel over weighted Monte Carlo samples (sxmc_kde_random_sample with
multiplicities): the device's events replayed draw by draw by tests/kde_sample_reference.draw with the pick replaced by
the weighted law of tests/kde_weighted_reference.py -- target = (word * T) >> 32, the first live row whose prefix sum
exceeds it -- under that module's rules for ambiguous draws; the planted picks must fail the same comparison."""
import numpy as np
import pytest

from sxmc_amd import pdfz
from sxmc_amd.mcmc import make_systematic
from tests import kde_sample_reference as KS
from tests import kde_weighted_reference as W
from tests.test_gpu_kde import gpu_kde

pytestmark = pytest.mark.gpu

LOWER, UPPER = -2.0, 2.0
SHIFT = {0: 0.5}
NEVENTS = 3000


def pool_table(rng, D, N, live, m_of_live):
    """N rows inside the domain that stay inside under the shift, `live` of them with the given multiplicities, and one
    more live row that the shift moves out (construction needs two; the pool then has `live`)."""
    t = rng.uniform(-1.5, 1.0, (N + 1, D)).astype(np.float32)
    t[N, 0] = 1.9
    m = np.zeros(N + 1, np.uint32)
    rows = np.sort(rng.choice(N, live, replace=False))
    m[rows] = m_of_live
    m[N] = 2
    return t, m


def sampled(table, D, m, alpha=0.0, shared=False):
    lower, upper = np.full(D, LOWER), np.full(D, UPPER)
    ev = pdfz.EvalKernel(table.ravel(), D, D, lower, upper, np.full(D, 0.7), dataset=2, bandwidth_sensitivity=alpha,
                         multiplicities=m)
    systs = [dict(type="shift", obs=0, pars=[0])]
    ev.AddSystematic(make_systematic(systs[0]))
    keep = [ev]
    if shared:
        ev = pdfz.EvalKernel.Shared(ev)
        keep.append(ev)
    pts = np.zeros((4, D + 1), np.float32)
    pts[:, D] = 2
    got = gpu_kde(None, None, D, lower, upper, None, None, SHIFT, pts.ravel(), ev=ev, do_eval_pdf=False)
    h, lam = ev.Bandwidths(), ev.LocalFactors()
    rows_c, row_index, fragile, cum = W.prepare_weighted(table, D, D, lower, upper, h, m, systs, SHIFT)
    assert got["norm"] == int(cum[-1]) and ev.SamplePool() == len(cum)
    return ev, keep, (rows_c, row_index, cum, lam, h, lower, upper), fragile


def check(ev, replay_args, fragile, label, lowers=None, uppers=None, seed=2 ** 33 + 5, nevents=NEVENTS):
    d = W.draw_weighted(*replay_args, nevents, seed, lowers, uppers, dataset=2, fragile=fragile)
    assert d["exhausted"] == 0
    got = ev.RandomSample(nevents, seed, lowers, uppers)
    res = KS.compare(got, d, label)
    assert res["ok"], res
    return got, d


@pytest.mark.parametrize("live", [1, 2, 255, 256, 257])
def test_pools_around_a_tile(live):
    rng = np.random.default_rng(40 + live)
    D = 1 if live % 2 else 2
    t, m = pool_table(rng, D, 700, live, [1, 4] if live == 2 else rng.integers(1, 6, live))
    ev, keep, args, fragile = sampled(t, D, m)
    assert len(args[2]) == live
    got, d = check(ev, args, fragile, "pool %d" % live)
    assert set(np.unique(d["row"])) <= set(np.flatnonzero(m > 0)[:-1].tolist())
    if live > 1:
        # the planted picks fail the comparison the device's events pass
        for plant in W.PICK_PLANTS:
            bad = W.draw_weighted(*args, NEVENTS, 2 ** 33 + 5, dataset=2, fragile=fragile, plant=plant)
            res = KS.compare(got, bad, "pool %d, planted %s" % (live, plant))
            if plant == "uniform" or live <= 2:
                assert not res["ok"], plant
    for e in keep:
        e.close()


def test_planted_first_ge_is_caught_where_targets_hit_prefix_sums():
    """Two live rows of multiplicity 1: half the targets sit on the first prefix sum, which tells `first C > target` from
    `first C >= target`."""
    rng = np.random.default_rng(9)
    t, m = pool_table(rng, 1, 300, 2, [1, 1])
    ev, keep, args, fragile = sampled(t, 1, m)
    got, _ = check(ev, args, fragile, "two rows of one")
    bad = W.draw_weighted(*args, NEVENTS, 2 ** 33 + 5, dataset=2, fragile=fragile, plant="first_ge")
    assert not KS.compare(got, bad, "planted first_ge")["ok"]
    for e in keep:
        e.close()


@pytest.mark.parametrize("alpha,shared", [(0.0, False), (0.5, True)], ids=["fixed", "adaptive_shared"])
def test_one_row_dominates(alpha, shared):
    rng = np.random.default_rng(77)
    t, m = pool_table(rng, 2, 400, 300, rng.integers(1, 4, 300))
    big = int(np.flatnonzero(m > 0)[123])
    m[big] = 2 ** 31
    ev, keep, args, fragile = sampled(t, 2, m, alpha, shared)
    got, d = check(ev, args, fragile, "one row of 2^31")
    share = float(np.mean(d["row"] == big))
    print("the dominating row is picked by %.4f of the events" % share)
    assert share > 0.99
    for e in keep:
        e.close()


def test_total_at_the_top_of_32_bits():
    """Two live rows of 2^31 - 1 and 2^31, every other row 0 (T = 2^32 - 1, the largest total an evaluator takes): the
    scan and the 64-bit product must not wrap."""
    rng = np.random.default_rng(3)
    t = rng.uniform(-1.5, 1.0, (300, 1)).astype(np.float32)
    m = np.zeros(300, np.uint32)
    m[40], m[260] = 2 ** 31 - 1, 2 ** 31
    ev, keep, args, fragile = sampled(t, 1, m)
    assert int(args[2][-1]) == 2 ** 32 - 1
    got, d = check(ev, args, fragile, "T = 2^32 - 1")
    first = float(np.mean(d["row"] == 40))
    assert 0.45 < first < 0.55 and set(np.unique(d["row"])) == {40, 260}
    for e in keep:
        e.close()


def test_a_cluster_of_zeros_yields_no_event_and_cuts_force_redraws():
    rng = np.random.default_rng(12)
    t, m = pool_table(rng, 1, 600, 400, rng.integers(1, 4, 400))
    cluster = np.flatnonzero((t[:, 0] > 0.2) & (t[:, 0] < 0.6))
    m[cluster] = 0
    assert len(cluster) > 30
    ev, keep, args, fragile = sampled(t, 1, m)
    _, d = check(ev, args, fragile, "a cluster of zeros")
    assert not np.isin(d["row"], cluster).any()
    lo, hi = np.array([-0.4], np.float32), np.array([0.9], np.float32)
    _, d = check(ev, args, fragile, "cuts", lo, hi)
    assert d["attempts"].max() > 2
    for e in keep:
        e.close()
