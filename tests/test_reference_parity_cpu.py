"""The CPU oracle held to what the fitted code's own compiled CPU-mode translation units compute.

tests/golden/reference_parity.json holds, for the cases of tests/reference_cases.py, the results of oracle/ref/'s
driver: the fitted code's pdfz and NLL translation units built unmodified (g++ -DHEMI_CUDA_DISABLE) against stand-in
headers, each case also run clean under ASan + UBSan.  The oracle (oracle/sxmc_oracle.c) is compiled with the same
arithmetic flags against the same libm, so everything here is compared BIT FOR BIT: a difference is a finding to explain,
not a tolerance to widen.

Also here: the fixture's log of random calls against what tests/step_reference.py assumes about a step's draws, the
conditions on the generator's undefined-behaviour filter, a fresh run of the driver against the committed file (skipped
only where the driver is not built), and negative controls: seven plausible misreadings of the fitted code, each of
which must disagree with the records on at least one named case.
"""
import os

import numpy as np
import pytest

from oracle import oracle
from tests import reference_cases as R
from tests import step_reference as SR
from tests.golden import make_reference_parity as REC


@pytest.fixture(scope="module")
def fixture():
    return R.load(REC.FIXTURE)      # (requires the regenerated inputs to be the recorded ones, by digest)


def nll_of(fixture, op):
    got = [(c, r) for c, r in fixture["nll"] if c["op"] == op]
    assert got
    return got


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        k = next(i for i in range(g.size) if g[i].tobytes() != w[i].tobytes())
        got, want = g, w
        raise AssertionError("%s: first difference at %d: got %r, recorded %r" % (what, k, got[k], want[k]))


# ---------------------------------------------------------------------------------------------- the fixture itself
def test_fixture_is_what_the_generators_make(fixture):
    """R.load() has regenerated every case and required the recorded digest of its inputs: the generators are stable
    and the records are paired with the inputs they were computed on."""
    assert len(fixture["pdfz"]) == len(fixture["raw"]["pdfz"]) == 50 and len(fixture["nll"]) == 97


def test_filter_conditions_and_no_undefined_input(fixture):
    """At most 2 % of a case's rows and points replaced, at least 10 rows left of the kind the case was built for,
    and, by the double-precision model on the COMMITTED inputs, no field that is NaN at the domain test and no flat
    index outside the histogram; every scripted queue used up exactly."""
    kinds = set()
    for (case, _), j in zip(fixture["pdfz"], fixture["raw"]["pdfz"]):
        n, m = case["samples"].shape[0], case["points"].shape[0]
        assert 0 < n <= R.MAX_SAMPLES and 0 < m <= R.MAX_POINTS, case["name"]
        assert j["replaced"] <= R.MAX_REPLACED_SHARE * n, case["name"]
        assert j["points_replaced"] <= R.MAX_REPLACED_SHARE * m, case["name"]
        assert j["built"] >= R.MIN_BUILT_ROWS, case["name"]
        geom = R.geometry(case)
        assert not any(R.row_is_undefined(case, row, geom) for row in case["samples"]), case["name"]
        assert not any(R.point_is_undefined(case, pt, geom) for pt in case["points"]), case["name"]
        kinds.add(case["kind"])
    assert kinds == {"random", "edge", "moved_edge", "special", "inner_nbins"}
    assert any(j["replaced"] > 0 for j in fixture["raw"]["pdfz"]), "the filter was never exercised"
    for case, res in fixture["pdfz"]:       # wild coefficients with some rows still inside, not only an empty histogram
        if case["name"].startswith("pars-wild"):
            assert res["norm"][case["norm_offset"]] >= 10, case["name"]
    for case, res in fixture["nll"]:
        assert res["rng_left"][0] == 0, case["name"]
        assert case.get("ne", 0) <= R.MAX_EVENTS


def test_inner_index_cases_are_what_they_claim(fixture):
    """The rows built for it do get an inner index equal to nbins with the flat index inside the histogram."""
    for case, _ in fixture["pdfz"]:
        if case["kind"] == "inner_nbins":
            assert R.model_fill(case)[2] >= R.MIN_BUILT_ROWS, case["name"]


# ---------------------------------------------------------------------------------------------- oracle: pdfz
def oracle_pdfz(case):
    geom = oracle.HistGeometry(case["lower"], case["upper"], case["nbins"])
    rb = oracle.set_eval_points(geom, case["points"], case["dataset"])
    bins, norm = oracle.bin_samples(geom, case["samples"], case["nfields"], R.oracle_systs(case),
                                    case["params"][case["param_offset"]:], case["param_stride"])
    out = np.full(case["out_len"], R.SENTINEL, np.float32)
    oracle.eval_pdf(rb, bins, norm, geom.bin_volume, out=out, offset=case["out_offset"], stride=case["out_stride"])
    nbuf = np.full(case["norm_len"], 55, np.uint32)
    nbuf[case["norm_offset"]] = norm
    return dict(bins=bins, norm=nbuf, out=out, read_bins=rb, bin_volume=np.array([geom.bin_volume]),
                total_nbins=geom.total_nbins)


def test_oracle_pdfz_bit_for_bit(fixture):
    for case, res in fixture["pdfz"]:
        got = oracle_pdfz(case)
        assert got["total_nbins"] == res["total_nbins"], case["name"]
        for key in ("bin_volume", "read_bins", "bins", "norm", "out"):
            assert_bits(got[key], res[key], case["name"] + " " + key)
        # untouched slots of the output buffer are still the pre-fill
        touched = case["out_offset"] + case["out_stride"] * np.arange(case["points"].shape[0])
        rest = np.delete(res["out"], touched)
        assert np.all(rest == np.float32(R.SENTINEL)), case["name"]


# ---------------------------------------------------------------------------------------------- oracle: NLL
def oracle_chunks(c):
    """Into a pre-filled destination, so that a sum that is not written stays visible."""
    return oracle.nll_event_chunks(c["lut"], c["pars"], c["ne"], c["ns"], c["nexpected"], c["n_mc"], c["source_id"],
                                   c["norms"], out=c["sums"].copy())


def oracle_total(c, pars=None, events_total=None):
    return oracle.nll_total(c["pars"] if pars is None else pars, c["nsignals"], c["nsources"], c["means"], c["sigmas"],
                            c["events_total"] if events_total is None else events_total, c["nexpected"], c["n_mc"],
                            c["source_id"], c["norms"])


def test_oracle_chunks_bit_for_bit(fixture):
    for c, res in nll_of(fixture, "chunks"):
        assert_bits(oracle_chunks(c), res["sums"], c["name"])
    # with one lane over all events the sum of logs of positive numbers is never NaN: it is always written
    assert all(res["sums"][0] != R.SENTINEL for _, res in nll_of(fixture, "chunks"))


def test_oracle_reduce_and_total_bit_for_bit(fixture):
    for c, res in nll_of(fixture, "reduce"):
        assert_bits(oracle.nll_event_reduce(c["sums"]), res["total"], c["name"])
    for c, res in nll_of(fixture, "total"):
        assert_bits(np.array([oracle_total(c)]), res["nll"], c["name"])
    names = {c["name"]: res["nll"][0] for c, res in nll_of(fixture, "total")}
    for n in ("total-events-nan", "total-source-negative", "total-negative-source-after-nan-sigma"):
        assert names[n] == 1e18, n
    assert names["total-source-minus-zero"] != 1e18 and names["total-syst-negative"] != 1e18
    assert names["total-events-plus-inf"] == -np.inf and names["total-events-minus-inf"] == np.inf
    assert np.isnan(names["total-source-nan"]) and np.isnan(names["total-syst-nan"])


def test_oracle_decider_bit_for_bit(fixture):
    for c, res in nll_of(fixture, "decider"):
        st = {k: c[k].copy() for k in ("nll_current", "v_current", "accepted", "counter", "jump_buffer")}
        with np.errstate(over="ignore"):
            oracle.jump_decider(float(c["rng"][0]), st["nll_current"], c["nll_proposed"], st["v_current"], c["v_proposed"],
                                st["accepted"], st["counter"], st["jump_buffer"])
        for k, v in st.items():
            assert_bits(v, res[k], c["name"] + " " + k)
        assert list(res["rng_kind"]) == [0], c["name"]                     # one uniform, nothing else
    acc = {c["name"]: int(res["accepted"][0] - c["accepted"][0]) for c, res in nll_of(fixture, "decider")}
    for stem in ("uphill-half", "uphill-3", "uphill-tiny"):
        assert (acc["decider-%s-u-below" % stem], acc["decider-%s-u-at" % stem], acc["decider-%s-u-above" % stem]) == \
               (1, 1, 0), stem
    assert acc["decider-both-1e18"] == 1 and acc["decider-inf-minus-inf"] == 0 and acc["decider-proposed-nan"] == 0
    assert acc["decider-uphill-u-largest"] == 0 and acc["decider-uphill-far-u-zero"] == 1


def _spread(c, popped):
    """The popped normals as one z per parameter (0 for the parameters that draw none)."""
    z = np.zeros(c["jump_width"].size)
    z[np.flatnonzero(c["jump_width"] > 0)] = popped
    return z


def test_oracle_pick_bit_for_bit(fixture):
    """What this pins: which parameters draw (width > 0: not 0, not negative, not NaN), that a parameter that does not
    is copied, that the float width is widened to double before use, and the order of the draws.  The arithmetic
    mean + sigma * z itself is the stand-in generator's, chosen to be the device form's."""
    for c, res in nll_of(fixture, "pick"):
        free = np.flatnonzero(c["jump_width"] > 0)
        assert list(res["rng_kind"]) == [1] * free.size, c["name"]
        args = res["rng_args"].reshape(-1, 3)
        assert_bits(args[:, 0], c["v_current"][free], c["name"] + " means")
        assert_bits(args[:, 1], c["jump_width"][free].astype(np.float64), c["name"] + " sigmas")
        got = oracle.pick_new_vector(_spread(c, args[:, 2]), c["jump_width"], c["v_current"])
        assert_bits(got, res["v_proposed"], c["name"])


def oracle_combo(c, res):
    """The oracle's stages composed into whole steps, fed the draws in the order the fixture's log recorded them."""
    P, npart = c["nparameters"], c["npartial"]
    args = res["rng_args"].reshape(-1, 3)
    nfree = int(np.count_nonzero(c["jump_width"] > 0))
    st = {k: c[k].copy() for k in ("nll_current", "v_current", "v_proposed", "accepted", "counter", "jump_buffer")}
    trace, itrace = [], []
    for s in range(c["nsteps"]):
        draws = args[s * (1 + nfree):(s + 1) * (1 + nfree), 2]
        total = oracle.nll_event_reduce(c["sums"][s * npart:(s + 1) * npart])
        nll_prop = np.array([oracle_total(c, pars=st["v_proposed"], events_total=total)])
        with np.errstate(over="ignore"):
            oracle.jump_decider(float(draws[0]), st["nll_current"], nll_prop, st["v_current"], st["v_proposed"],
                                st["accepted"], st["counter"], st["jump_buffer"], bool(c["debug"]))
        st["v_proposed"] = oracle.pick_new_vector(_spread(c, draws[1:]), c["jump_width"], st["v_current"])
        trace += [st["nll_current"][0], nll_prop[0]] + list(st["v_current"]) + list(st["v_proposed"])
        itrace += [st["accepted"][0], st["counter"][0], (s + 1) * (1 + nfree)]
    return np.array(trace), np.array(itrace, np.int32), st["jump_buffer"]


def test_oracle_combo_bit_for_bit(fixture):
    for c, res in nll_of(fixture, "combo"):
        trace, itrace, jb = oracle_combo(c, res)
        assert_bits(trace, res["trace"], c["name"] + " trace")
        assert_bits(itrace, res["itrace"], c["name"] + " accepted / counter / draws")
        assert_bits(jb, res["jump_buffer"], c["name"] + " jump buffer")
    it = {c["name"]: res["itrace"].reshape(-1, 3) for c, res in nll_of(fixture, "combo")}
    assert list(it["combo-accept-reject-accept"][:, 0]) == [1, 1, 2]
    assert list(it["combo-debug"][:, 0]) == [1, 2, 3]
    # ... and "combo-debug" accepts a step that only debug mode accepts: its second step is uphill and the Metropolis
    # rule on the recorded uniform rejects it, so an oracle that dropped `debug_mode ||` would not reproduce the record
    c, res = next((c, r) for c, r in nll_of(fixture, "combo") if c["name"] == "combo-debug")
    tr = res["trace"].reshape(c["nsteps"], -1)
    u = res["rng_args"].reshape(-1, 3)[1 + int(np.count_nonzero(c["jump_width"] > 0)), 2]
    assert tr[1, 1] > tr[0, 0] and not R.model_decide(u, tr[0, 0], tr[1, 1], debug=False)
    assert tr[1, 0] == tr[1, 1] and R.model_decide(u, tr[0, 0], tr[1, 1], debug=True)
    plain = R.model_combo(dict(c, debug=0))
    assert not R.same_bits(plain[0], res["trace"]) and list(plain[1].reshape(-1, 3)[:, 0]) == [1, 1, 2]


# ---------------------------------------------------------------------------------------------- the draws of a step
def test_random_call_log_is_what_step_reference_assumes(fixture):
    """tests/step_reference.py: per step the decider's uniform first -- also when parameter 0 is fixed -- then one
    normal from every free parameter (width > 0) in index order, centred on the vector AFTER the decision, the float
    width widened to double; decide() and propose() give the recorded decisions and proposals."""
    for c, res in nll_of(fixture, "combo"):
        P = c["nparameters"]
        free = np.flatnonzero(c["jump_width"] > 0)
        kinds, args = res["rng_kind"], res["rng_args"].reshape(-1, 3)
        assert list(kinds) == ([0] + [1] * free.size) * c["nsteps"], c["name"]
        tr = res["trace"].reshape(c["nsteps"], 2 + 2 * P)
        nll_cur, accepted = c["nll_current"][0], int(c["accepted"][0])
        for s in range(c["nsteps"]):
            a = args[s * (1 + free.size):(s + 1) * (1 + free.size)]
            with np.errstate(invalid="ignore"):
                accept = SR.decide(a[0, 2], nll_cur, tr[s, 1], bool(c["debug"]))
            accepted += accept
            nll_cur = tr[s, 1] if accept else nll_cur
            assert accepted == res["itrace"].reshape(-1, 3)[s, 0], (c["name"], s)
            v_cur = tr[s, 2:2 + P]
            assert_bits(a[1:, 0], v_cur[free], "%s step %d means" % (c["name"], s))
            assert_bits(a[1:, 1], c["jump_width"][free].astype(np.float64), "%s step %d sigmas" % (c["name"], s))
            assert_bits(SR.propose(_spread(c, a[1:, 2]), c["jump_width"], v_cur), tr[s, 2 + P:],
                        "%s step %d proposal" % (c["name"], s))
    assert any(c["jump_width"][0] <= 0 < np.count_nonzero(c["jump_width"] > 0) for c, _ in nll_of(fixture, "combo"))
    for c, res in nll_of(fixture, "decider"):
        with np.errstate(invalid="ignore"):
            accept = SR.decide(float(c["rng"][0]), c["nll_current"][0], c["nll_proposed"][0])
        assert int(accept) == res["accepted"][0] - c["accepted"][0], c["name"]


# ---------------------------------------------------------------------------------------------- a fresh driver run
@pytest.mark.skipif(not os.path.exists(REC.DRIVER), reason="oracle/_ref/ref_driver is not built (no tree to build it from)")
def test_fresh_driver_run_reproduces_the_committed_fixture():
    """The committed file is what the fitted code's compiled translation units compute on the regenerated inputs, byte
    for byte.  (The recorder also runs the sanitizer build; this test runs the plain one, which it requires to agree.)"""
    with open(REC.FIXTURE) as f:
        committed = f.read()
    assert REC.dumps(REC.record(drivers=(REC.DRIVER,))) == committed


# ---------------------------------------------------------------------------------------------- negative controls
def disagreements(pairs):
    return sorted(name for name, same in pairs if not same)


def test_controls_pdfz(fixture):
    """The model as written agrees with every record; `x <= upper` and a clamped inner index do not."""
    le_upper, clamp = [], []
    for case, res in fixture["pdfz"]:
        bins, norm, _ = R.model_fill(case)
        assert np.array_equal(bins, res["bins"]) and norm == res["norm"][case["norm_offset"]], case["name"]
        assert np.array_equal(R.model_read_bins(case), res["read_bins"]), case["name"]
        b, n, _ = R.model_fill(case, "le_upper")
        le_upper.append((case["name"], np.array_equal(b, res["bins"]) and n == res["norm"][case["norm_offset"]]))
        b, n, _ = R.model_fill(case, "clamp")
        clamp.append((case["name"], np.array_equal(b, res["bins"]) and n == res["norm"][case["norm_offset"]]))
    print("x <= upper disagrees on:", disagreements(le_upper))
    print("inner index clamped to nbins - 1 disagrees on:", disagreements(clamp))
    assert "nbins-1" in disagreements(le_upper) and "tiny-domain" in disagreements(le_upper)
    assert {"inner-index-2d", "inner-index-3d-middle", "inner-index-4d-last"} <= set(disagreements(clamp))


def test_controls_nll(fixture):
    """`eff` kept in double, `s >= 0`, `sigma >= 0`, `u < exp(...)`, the uniform drawn after the normals: each
    disagrees with the records on named cases, while the model as written agrees with all of them."""
    eff, sge = [], []
    for c, res in nll_of(fixture, "chunks"):
        assert_bits(np.array([R.model_chunks(c, sentinel=R.SENTINEL)]), res["sums"], c["name"] + " (model)")
        eff.append((c["name"], R.same_bits(np.array([R.model_chunks(c, "eff_double", R.SENTINEL)]), res["sums"])))
        sge.append((c["name"], R.same_bits(np.array([R.model_chunks(c, "s_ge_0", R.SENTINEL)]), res["sums"])))
    sig = []
    for c, res in nll_of(fixture, "total"):
        assert_bits(np.array([R.model_total(c)]), res["nll"], c["name"] + " (model)")
        sig.append((c["name"], R.same_bits(np.array([R.model_total(c, "sigma_ge_0")]), res["nll"])))
    ult = []
    for c, res in nll_of(fixture, "decider"):
        u, nc, np_ = float(c["rng"][0]), float(c["nll_current"][0]), float(c["nll_proposed"][0])
        want = int(res["accepted"][0] - c["accepted"][0])
        assert int(R.model_decide(u, nc, np_)) == want, c["name"]
        ult.append((c["name"], int(R.model_decide(u, nc, np_, variant="u_lt")) == want))
    last = []
    for c, res in nll_of(fixture, "combo"):
        tr, it, jb = R.model_combo(c)
        assert_bits(tr, res["trace"], c["name"] + " (model)")
        assert_bits(it, res["itrace"], c["name"] + " (model)")
        assert_bits(jb, res["jump_buffer"], c["name"] + " (model)")
        tr, it, jb = R.model_combo(c, "uniform_last")
        last.append((c["name"], R.same_bits(tr, res["trace"]) and R.same_bits(jb, res["jump_buffer"])))
    for what, pairs in (("eff kept in double", eff), ("s >= 0", sge), ("sigma >= 0", sig), ("u < exp(nc - np)", ult),
                        ("the uniform drawn after the normals", last)):
        print(what, "disagrees on:", disagreements(pairs))
    assert "chunks-modes-ratio" in disagreements(eff) and "chunks-ne300-ns17-ratio" in disagreements(eff)
    assert "chunks-modes-zero-event" in disagreements(sge) and "chunks-modes-all-empty" in disagreements(sge)
    assert {"total-sigma-zero-all", "total-sigma-zero-off-mean", "total-sigma-zero-on-mean"} <= set(disagreements(sig))
    assert {"decider-uphill-half-u-at", "decider-uphill-3-u-at", "decider-uphill-tiny-u-at", "decider-uphill-far-u-zero"} <= set(disagreements(ult))
    assert {"combo-accept-reject-accept", "combo-parameter-0-fixed"} <= set(disagreements(last))
