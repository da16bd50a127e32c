"""The HIP library held directly to what the fitted code's own compiled CPU-mode translation units computed.

Reads only tests/golden/reference_parity.json and the inputs that tests/reference_cases.py regenerates for it (the
file names them by digest); never the fitted code's tree or anything compiled from it.  (How the file is recorded:
tests/golden/make_reference_parity.py, and tests/test_reference_parity_cpu.py holds the CPU oracle to the same records).

pdfz family: bins, norm buffer, output buffer and the table of read indices BIT FOR BIT, through a single
pdfz.EvalHist and through a group in every form of the fill that the plan accepts for the case (what the plan declines
is recorded from LaunchInfo(), never run twice under two names).

NLL family: every discrete outcome exact (the 1e18 returns, a result that is not finite, which slots were written,
counters, acceptance given the uniform the device drew); sums to NLL_RTOL (this project's 1e-12) times the SUM OF THE
ABSOLUTE VALUES OF THE TERMS, worked out here in double from the fixture's inputs -- not the result's magnitude, since
several edge cases cancel to near zero.  Only the summation order and the device's log differ from the records.  The
worst observed ratio to that tolerance is printed per family.
"""
import math
import os
import re

import numpy as np
import pytest

from oracle import oracle
from sxmc_amd import capi, nll, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests import reference_cases as R
from tests import step_reference as SR

same_bits = R.same_bits

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-12          # tests/test_gpu_nll.py
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_parity.json")
SHAPES = [(1, 64, 64), (3, 192, 256), (64, 256, 128)]          # (grid, block, reduce threads) of test_nll_launch_shapes


@pytest.fixture(scope="module")
def fixture():
    return R.load(FIXTURE)


def nll_of(fixture, op):
    got = [(c, r) for c, r in fixture["nll"] if c["op"] == op]
    assert got
    return got


class Worst:
    """The worst ratio |got - recorded| / tolerance of a family, and where."""

    def __init__(self, family):
        self.family, self.ratio, self.where = family, 0.0, None

    def check(self, got, want, abs_terms, where):
        """Exact where the record is not finite or is the 1e18 penalty; else within NLL_RTOL * abs_terms."""
        got, want = float(got), float(want)
        if not math.isfinite(want) or want == 1e18:
            assert got == want or (got != got and want != want), (where, got, want)
            return
        assert math.isfinite(got), (where, got, want)
        tol = NLL_RTOL * abs_terms
        err = abs(got - want)
        if err > 0:
            assert tol > 0 and err <= tol, (where, got, want, err, tol)
            if err / tol > self.ratio:
                self.ratio, self.where = err / tol, where

    def report(self):
        print("worst |device - recorded| / (%g * sum |terms|) over %s: %.3g%s"
              % (NLL_RTOL, self.family, self.ratio, " (%s)" % (self.where,) if self.where else ""))


# ---------------------------------------------------------------------------------------------- pdfz
def make_evaluator(case):
    ev = pdfz.EvalHist(case["samples"], case["nfields"], case["nobs"], case["lower"], case["upper"], case["nbins"],
                       dataset=case["dataset"])
    for kind, obs, extra, pars in case["systs"]:
        ev.AddSystematic(make_systematic(dict(type=R.KIND_NAME[kind], obs=obs, true_obs=extra, pars=pars)))
    bufs = dict(out=DeviceArray(np.full(case["out_len"], R.SENTINEL, np.float32)),
                norm=DeviceArray(np.full(case["norm_len"], 55, np.uint32)), params=DeviceArray(case["params"].copy()))
    ev.SetEvalPoints(case["points"])
    ev.SetPDFValueBuffer(bufs["out"], case["out_offset"], case["out_stride"])
    ev.SetNormalizationBuffer(bufs["norm"], case["norm_offset"])
    ev.SetParameterBuffer(bufs["params"], case["param_offset"], case["param_stride"])
    return ev, bufs


def check_pdfz(case, res, ev, bufs, evaluate, where):
    """One evaluation for look-up against the records; the dense histogram from an evaluation without look-up where
    the first counted the event bins only (a histogram beyond LDS)."""
    bufs["out"].set(np.full(case["out_len"], R.SENTINEL, np.float32))
    bufs["norm"].set(np.full(case["norm_len"], 55, np.uint32))
    evaluate(True)
    assert same_bits(bufs["norm"].get(), res["norm"]), (where, "norm", bufs["norm"].get(), res["norm"])
    assert same_bits(bufs["out"].get(), res["out"]), (where, "values")
    assert same_bits(ev.GetReadBins(), res["read_bins"]), (where, "read_bins")
    try:
        bins = ev.GetBins()
    except capi.SxmcError:
        evaluate(False)
        bins = ev.GetBins()
        assert same_bits(bufs["norm"].get(), res["norm"]), (where, "norm of the dense fill")
    assert np.array_equal(bins, res["bins"]), (where, "bins", np.flatnonzero(bins != res["bins"])[:8])
    assert ev.total_nbins == res["total_nbins"] and ev.bin_volume == res["bin_volume"][0], (where, "geometry")


def test_single_evaluator_bit_for_bit(fixture):
    for case, res in fixture["pdfz"]:
        ev, bufs = make_evaluator(case)

        def evaluate(lookup):
            ev.EvalAsync(lookup)
            ev.EvalFinished()
        check_pdfz(case, res, ev, bufs, evaluate, case["name"])
        ev.close()


# name -> (prebinning, bucketing, ordering (forced), boxes, codes)
FORMS = {"plain": (False, False, False, False, False), "prebinned": (True, False, False, False, False),
         "bucketed": (True, True, False, False, False), "ordered": (True, True, True, False, False),
         "codes": (True, True, True, False, True), "boxed": (True, True, True, True, None)}


def launches_of(info):
    """What LaunchInfo() says is launched: per launch (hist, program, table)."""
    out = []
    for line in re.findall(r"^launch \d+: (.*)$", info, re.M):
        f = dict(kv.split("=", 1) for kv in line.split())
        out.append((f["hist"], f["program"], f["table"]))
    return tuple(out)


def test_group_forms_bit_for_bit(fixture):
    """Every case through a one-member group, the plan steered to each form, run-time kernels on and off.  A setting
    whose plan is one already run for the case is recorded as declined and not run again."""
    ran, declined = {}, {}
    for case, res in fixture["pdfz"]:
        ev, bufs = make_evaluator(case)
        group = nll.EvalGroup([ev])
        seen = set()

        def evaluate(lookup):
            group.EvalAsync(lookup)
            group.EvalFinished()
        for rtc in (False, True):
            for form, (pre, bucket, order, boxes, codes) in FORMS.items():
                group.SetRuntimeKernels(rtc)
                group.SetPrebinning(pre)
                group.SetBucketing(bucket)
                group.SetOrdering(order, force=True)
                group.SetBoxes(boxes)
                group.SetCodes(codes)
                info = group.LaunchInfo()
                plan = launches_of(info)
                assert plan and "failed" not in info, (case["name"], form, rtc, info)
                if plan in seen:
                    declined.setdefault((form, rtc), []).append(case["name"])
                    continue
                seen.add(plan)
                check_pdfz(case, res, ev, bufs, evaluate, (case["name"], form, "rtc" if rtc else "no rtc", plan))
                for launch in plan:
                    ran.setdefault(launch, []).append(case["name"])
        group.close()
        ev.close()
    for launch in sorted(ran):
        print("ran hist=%s program=%s table=%s on %d cases" % (launch + (len(ran[launch]),)))
    for key in sorted(declined, key=str):
        print("form %s, run-time kernels %s: the plan was one already run on %d cases"
              % (key[0], "on" if key[1] else "off", len(declined[key])))
    tables = {t.split("+")[0].split("|")[0] for _, _, t in ran}
    assert {"rows", "prebinned", "bucketed", "ordered", "boxed"} <= tables, tables
    assert any(t.startswith("ordered+codes") for _, _, t in ran), sorted(ran)
    assert {"builtin", "runtime", "decoded"} <= {p for _, p, _ in ran}, sorted(ran)


# ---------------------------------------------------------------------------------------------- NLL: separate launch points
def event_terms(c):
    """sum over events of |log s| for s > 0 (in double, the record's own arithmetic)."""
    ne, ns = c["ne"], c["ns"]
    with np.errstate(all="ignore"):
        eff = (np.float64(1.0) * c["norms"] / c["n_mc"]).astype(np.float32).astype(np.float64)
        w = c["pars"][c["source_id"]] * c["nexpected"] * eff
        lut = c["lut"].reshape(ns, ne).astype(np.float64)
        lut = np.where(np.isnan(lut), 0.0, lut)
        s = np.zeros(ne)
        for j in range(ns):
            s = s + w[j] * lut[j]
        logs = np.log(s[s > 0])
    return float(np.sum(np.abs(logs[np.isfinite(logs)])))


def total_terms(c, pars, events_total):
    with np.errstate(all="ignore"):
        t = abs(float(events_total))
        t += float(np.sum(np.abs(pars[c["source_id"]] * c["nexpected"] * c["norms"] / c["n_mc"])))
        sg = c["sigmas"]
        ok = sg > 0
        t += float(np.sum(0.5 * ((pars[ok] - c["means"][ok]) / sg[ok]) ** 2))
    return t


def dev(c, *keys):
    return {k: DeviceArray(c[k].copy()) for k in keys}


def test_event_sum_launch_points(fixture):
    worst = Worst("nll_event_chunks + nll_event_reduce")
    for c, res in nll_of(fixture, "chunks"):
        d = dev(c, "lut", "pars", "nexpected", "n_mc", "source_id", "norms")
        terms = event_terms(c)
        for grid, block, red in SHAPES:
            sums = DeviceArray(np.full(grid * block, 1e300))          # stale garbage must be overwritten
            total = DeviceArray(np.full(1, R.SENTINEL))
            nll.nll_event_chunks(grid, block, None, d["lut"], d["pars"], c["ne"], c["ns"], d["nexpected"], d["n_mc"],
                                 d["source_id"], d["norms"], sums)
            nll.nll_event_reduce(1, red, None, grid * block, sums, total)
            capi.synchronize()
            assert not np.any(sums.get() == 1e300), (c["name"], "a lane did not write its partial sum")
            worst.check(total.get()[0], res["sums"][0], terms, (c["name"], grid, block, red))
    worst.report()
    worst = Worst("nll_event_reduce")
    for c, res in nll_of(fixture, "reduce"):
        sums = DeviceArray(c["sums"].copy())
        with np.errstate(invalid="ignore"):
            terms = float(np.sum(np.abs(c["sums"][np.isfinite(c["sums"])])))
        for _, _, red in SHAPES:
            total = DeviceArray(np.full(1, R.SENTINEL))
            nll.nll_event_reduce(1, red, None, c["sums"].size, sums, total)
            capi.synchronize()
            worst.check(total.get()[0], res["total"][0], terms, (c["name"], red))
    worst.report()


def test_nll_total_launch_point(fixture):
    worst = Worst("nll_total")
    for c, res in nll_of(fixture, "total"):
        d = dev(c, "pars", "means", "sigmas", "events_total", "nexpected", "n_mc", "source_id", "norms")
        out = DeviceArray(np.full(1, R.SENTINEL))
        nll.nll_total(1, 1, None, c["nparameters"], d["pars"], c["nsignals"], c["nsources"], d["means"], d["sigmas"],
                      d["events_total"], d["nexpected"], d["n_mc"], d["source_id"], d["norms"], out)
        capi.synchronize()
        worst.check(out.get()[0], res["nll"][0], total_terms(c, c["pars"], c["events_total"][0]), c["name"])
    worst.report()


def test_jump_decider_launch_point(fixture):
    """The device draws its own uniform (generator 0 of the seed, first draw): the decision must be the recorded RULE
    on that uniform, the state what the oracle -- held bit for bit to the records -- makes of it; and where that is the
    recorded decision, the recorded state bit for bit."""
    same_as_recorded = 0
    for k, (c, res) in enumerate(nll_of(fixture, "decider")):
        P, seed = c["nparameters"], 1000 + k
        u = SR.word_to_uniform(SR.generator_words(seed, 0, 0)[0])
        rngs = nll.make_rngs(P, seed)
        d = dev(c, "nll_current", "nll_proposed", "v_current", "v_proposed", "accepted", "counter", "jump_buffer")
        nll.jump_decider(1, 64, None, rngs, d["nll_current"], d["nll_proposed"], d["v_current"], d["v_proposed"], P,
                         d["accepted"], d["counter"], d["jump_buffer"])
        capi.synchronize()
        want = {key: c[key].copy() for key in ("nll_current", "v_current", "accepted", "counter", "jump_buffer")}
        with np.errstate(all="ignore"):
            accept = SR.decide(u, c["nll_current"][0], c["nll_proposed"][0])
            oracle.jump_decider(u, want["nll_current"], c["nll_proposed"], want["v_current"], c["v_proposed"],
                                want["accepted"], want["counter"], want["jump_buffer"])
        assert want["accepted"][0] - c["accepted"][0] == int(accept), c["name"]
        recorded = int(res["accepted"][0] - c["accepted"][0]) == int(accept)
        same_as_recorded += recorded
        for key, w in want.items():
            assert same_bits(d[key].get(), w), (c["name"], key, d[key].get(), w)
            if recorded:
                assert same_bits(d[key].get(), res[key]), (c["name"], key, "the record")
        st = rngs.get().reshape(P, 4)
        assert st[0, 2] == 1 and np.all(st[1:, 2] == 0), (c["name"], "draws taken")
    assert same_as_recorded >= 15


def test_pick_new_vector_launch_point(fixture):
    """Exact: a parameter whose width is not > 0 (zero, negative, NaN) is copied and draws nothing.  The free ones:
    current + (double) width * z with z the device's own normal, to the proposal's rounding."""
    for k, (c, res) in enumerate(nll_of(fixture, "pick")):
        n, seed = c["n"], 2000 + k
        rngs = nll.make_rngs(n, seed)
        d = dev(c, "jump_width", "v_current", "v_proposed")
        nll.pick_new_vector(1, 64, None, n, rngs, d["jump_width"], d["v_current"], d["v_proposed"])
        capi.synchronize()
        got, free = d["v_proposed"].get(), c["jump_width"] > 0
        assert same_bits(got[~free], c["v_current"][~free]) and same_bits(got[~free], res["v_proposed"][~free]), c["name"]
        st = rngs.get().reshape(n, 4)
        assert np.array_equal(st[:, 2], free.astype(np.uint64)), (c["name"], "draws taken")
        z = np.zeros(n)
        for i in np.flatnonzero(free):
            w = SR.generator_words(seed, int(i), 0)
            z[i] = SR.words_to_normal(w[0], w[1])
        want = SR.propose(z, c["jump_width"], c["v_current"])
        tol = 1e-12 * np.abs(c["jump_width"].astype(np.float64)) * np.maximum(1.0, np.abs(z)) + 4e-16 * np.abs(want)
        assert np.all(np.abs(got[free] - want[free]) <= tol[free]), (c["name"], got, want)


# ---------------------------------------------------------------------------------------------- NLL: whole steps
def test_finish_combo_in_debug_mode(fixture):
    """Three steps on carried state in debug mode (every step accepted).  The first step's NLL is the record's own;
    the later ones are taken at the device's own proposals, so they are held to the oracle at those vectors."""
    worst = Worst("finish_nll_jump_pick_combo")
    for k, (c, res) in enumerate(nll_of(fixture, "combo")):
        P, npart, seed = c["nparameters"], c["npartial"], 3000 + k
        rngs = nll.make_rngs(P, seed)
        d = dev(c, "means", "sigmas", "nll_current", "nll_proposed", "v_current", "v_proposed", "accepted", "counter",
                "jump_buffer", "jump_width", "nexpected", "n_mc", "source_id", "norms")
        free = c["jump_width"] > 0
        tr = res["trace"].reshape(c["nsteps"], 2 + 2 * P)
        for s in range(c["nsteps"]):
            part = c["sums"][s * npart:(s + 1) * npart]
            sums = DeviceArray(part.copy())
            proposal = d["v_proposed"].get()
            if s == 0:
                assert same_bits(proposal, c["v_proposed"])
            nll.finish_nll_jump_pick_combo(1, 128, None, npart, sums, c["nsignals"], c["nsources"], d["means"],
                                           d["sigmas"], rngs, d["nll_current"], d["nll_proposed"], d["v_current"],
                                           d["v_proposed"], d["accepted"], d["counter"], d["jump_buffer"], P,
                                           d["jump_width"], d["nexpected"], d["n_mc"], d["source_id"], d["norms"], True)
            capi.synchronize()
            where = (c["name"], "step", s)
            total = oracle.nll_event_reduce(part)
            want = oracle.nll_total(proposal, c["nsignals"], c["nsources"], c["means"], c["sigmas"], total,
                                    c["nexpected"], c["n_mc"], c["source_id"], c["norms"])
            if s == 0:
                assert same_bits(np.array([want]), tr[0, 1:2]), where                  # the oracle IS the record here
            got = d["nll_proposed"].get()[0]
            with np.errstate(invalid="ignore"):
                terms = float(np.sum(np.abs(part[np.isfinite(part)]))) + total_terms(c, proposal, 0.0)
            worst.check(got, want, terms, where)
            # discrete: accepted, appended, the row is the proposal and its NLL as floats, the rest untouched
            assert d["accepted"].get()[0] == s + 1 and d["counter"].get()[0] == s + 1, where
            assert same_bits(d["v_current"].get(), proposal) and same_bits(d["nll_current"].get(), np.array([got])), where
            jb = d["jump_buffer"].get()
            with np.errstate(over="ignore"):
                row = np.concatenate([proposal.astype(np.float32), np.array([got], np.float64).astype(np.float32)])
            assert same_bits(jb[s * (P + 1):(s + 1) * (P + 1)], row), where
            assert np.all(jb[(s + 1) * (P + 1):] == np.float32(R.SENTINEL)), where
            # the next proposal: fixed parameters copied, free ones moved; one uniform, then one normal per free one
            nxt = d["v_proposed"].get()
            assert same_bits(nxt[~free], proposal[~free]), where
            st = rngs.get().reshape(P, 4)
            draws = (s + 1) * free.astype(np.uint64)
            draws[0] += s + 1
            assert np.array_equal(st[:, 2], draws), (where, "draws taken", st[:, 2])
    worst.report()
