"""CPU model of the BOXED fill's two arguments (fill_boxed_body, sxmc_amd/csrc/fill_kernels.inc.h), on rows built to
test them.  No GPU: the arguments themselves are what is tested.

tests/boxed_reference.py restates (a) the boxed copy of THE BOUND -- one streamed field binned from a 16-bit code when
fract(u') >= thr -- and (b) the interval rule -- the reference's operations on the corners of a granule's box, "one
bin" when both ends agree.  tests/boxed_rows.py builds the inputs that meet either condition: rows filling the code
cells around every bin edge with the parameter solved so that an edge sits a few float spacings inside a cell
boundary, and clusters whose box corners are rows with one corner's image solved onto an edge.  Held here against the
reference's per-row arithmetic (reference_bins of tests/test_codes_model_cpu.py, tied to oracle.bin_samples there and
below):
  * every row the model trusts is in the bin, or outside the domain, exactly as the reference has it;
  * every granule the model decides "one bin" or "skip" has all its rows there;
  * the inputs have teeth: a halved threshold misplaces rows, each planted variant of the interval rule decides a
    granule wrongly -- so a kernel with such a mistake does not get past tests/test_gpu_boxed_threshold.py;
  * the tables do not test nothing: the share of rows trusted and of granules decided is held at a floor."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import boxed_reference as model
from tests import boxed_rows as rows

from tests.boxed_rows import DECIDED_FLOOR, TRUSTED_FLOOR      # (beside the builders: the GPU worker holds the device to them)


@functools.lru_cache(maxsize=None)
def threshold_table(name):
    return rows.threshold_table(name)


@functools.lru_cache(maxsize=None)
def corner_table(name):
    t = rows.corner_table(name)
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    t["groups"], t["boxes"] = model.layout_granules(t["tab"], rows.BOXED, rows.TRUTH, [spec["unwritten"]], lo, hi, nb)
    return t


def threshold_counts(t, params, **scales):
    """(rows trusted, trusted rows the reference has elsewhere, built rows, built rows trusted) at one parameter vector."""
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    s = spec["streamed"]
    codes = t.setdefault("codes", model.encode16(t["tab"][:, s], t["base"], t["step"]))
    bound = model.streamed_bound(spec["systs"], params, s, t["base"], t["step"], lo[s], hi[s], nb[s], **scales)
    assert bound["ok"], (t["name"], params)
    idx, trusted, inside, queued = model.classify_codes(codes, bound)
    idx_ref, _, ind_k = model.reference_bins(t["tab"], spec["systs"], params, lo, hi, nb)
    wrong = trusted & ((inside != ind_k[s]) | (inside & (idx != idx_ref[s])))
    return int(trusted.sum()), int(wrong.sum()), int(t["built"].sum()), int((trusted & t["built"]).sum())


@pytest.mark.parametrize("name", ["c3-shift", "scale-positive", "scale-negative", "ctscale-streamed", "shift-after-scale"])
def test_trusted_rows_on_the_threshold_land_where_the_reference_puts_them(name):
    t = threshold_table(name)
    nedges = t["spec"]["geom"][2][t["spec"]["streamed"]] + 1
    # (3 cells x 2 sides x 6 spacings per edge; a scale does not move the edge at 0, a cos-theta scale the one at 1)
    assert len(t["params"]) >= 36 * (nedges - 1) and int(t["built"].sum()) > 2000 * nedges, (len(t["params"]), int(t["built"].sum()))
    wrong = wrong_half = wrong_85 = trusted_built = built = 0
    for i, params in enumerate(t["params"]):
        ntr, nwrong, nbuilt, ntb = threshold_counts(t, params)
        wrong += nwrong
        trusted_built += ntb
        built += nbuilt
        if i % 4 == 0:                                              # (the controls: on a quarter of the evaluations)
            wrong_half += threshold_counts(t, params, total_scale=0.5)[1]
            wrong_85 += threshold_counts(t, params, total_scale=model.dbg_scale(0.85)[1])[1]
    share = trusted_built / built
    print("%s: %d evaluations, %d built rows, trusted share %.4f; wrongly binned: %d as shipped, %d at 0.85, %d at 0.5"
          % (name, len(t["params"]), int(t["built"].sum()), share, wrong, wrong_85, wrong_half))
    assert wrong == 0
    # the built rows have teeth: a threshold half (even 85 %) of the bound misplaces them
    assert wrong_half > 1000 and wrong_85 > 0, (wrong_half, wrong_85)
    # ... and the bound does not buy its safety by trusting nothing
    assert share > TRUSTED_FLOOR[name], share


def test_what_the_roundings_share_is_worth_with_one_field():
    """Everything but Q scaled to 0 (rounding_scale): with ONE field nearly every row between a cell boundary and an edge
    is still covered by the half step alone (a handful of 50 000 rows go wrong) -- printed, because it bounds what the
    GPU measurement of the boxed form's margin (tests/boxed_margin_worker.py: s_min) can show."""
    t = threshold_table("c3-shift")
    wrong = sum(threshold_counts(t, p, rounding_scale=0.0)[1] for p in t["params"][::4])
    half = sum(threshold_counts(t, p, total_scale=0.5)[1] for p in t["params"][::4])
    print("c3-shift: wrongly binned with the roundings' share at 0: %d (threshold halved: %d)" % (wrong, half))
    # e = Q alone is still above half of 1.01 (Q + S + D): the roundings' share is worth no more than that
    assert wrong < half


def corner_verdicts(t, variant=None):
    """Over every solved parameter vector: (granules decided, granules decided WRONGLY, granules, rows of granules
    decided at the base parameters / rows)."""
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    b = rows.BOXED
    decided = wrong = total = 0
    cache = t.setdefault("reference", {})
    for i, params in enumerate(t["params"]):
        if i not in cache:
            idx_ref, _, ind_k = model.reference_bins(t["tab"], spec["systs"], params, lo, hi, nb)
            cache[i] = (idx_ref[b], ind_k[b])
        idx_b, ind_b = cache[i]
        verdict, e0 = model.granule_verdict(t["boxes"], spec["systs"], params, b, rows.TRUTH, lo[b], hi[b], nb[b],
                                            variant=variant)
        for g in np.flatnonzero(verdict != model.MIXED):
            r = t["groups"][g]
            if verdict[g] == model.SKIP:
                ok = not ind_b[r].any()
            else:
                ok = bool(ind_b[r].all()) and bool(np.all(idx_b[r] == e0[g]))
            wrong += 0 if ok else 1
        decided += int(np.sum(verdict != model.MIXED))
        total += verdict.size
    return decided, wrong, total


def decided_share(t):
    """The share of the table's in-domain rows in granules decided without the float path, at the base parameters."""
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    return model.decided_row_share(t["tab"], t["groups"], t["boxes"], spec["systs"], spec["base"], rows.BOXED, rows.TRUTH,
                                   lo, hi, nb)


@pytest.mark.parametrize("name", list(rows.CORNER_PROGRAMS))
def test_granules_decided_from_their_box_hold_all_their_rows(name):
    t = corner_table(name)
    assert len(t["params"]) >= 150, len(t["params"])
    ends = {s["edge"] for s in t["solved"]}
    nbx = t["spec"]["geom"][2][rows.BOXED]
    assert 0 in ends and nbx in ends and {s["corner"] for s in t["solved"]} == set(rows.CORNERS)
    decided, wrong, total = corner_verdicts(t)
    share = decided_share(t)
    print("%s: %d granules x %d evaluations, %d decided, %d wrongly; decided at the base parameters: %.3f"
          % (name, t["boxes"].shape[0], len(t["params"]), decided, wrong, share))
    assert wrong == 0
    assert share > DECIDED_FLOOR[name], share


def test_each_planted_variant_of_the_interval_rule_decides_granules_wrongly():
    caught = {}
    for variant in model.VARIANTS:
        caught[variant] = {name: corner_verdicts(corner_table(name), variant)[1] for name in rows.CORNER_PROGRAMS}
    print("granules decided wrongly, per variant and table: %r" % caught)
    for variant, by_table in caught.items():
        assert sum(by_table.values()) > 0, variant
    # where each mistake lives: the sign it forgets, the corner it mixes up
    assert caught["no_swap_negative_scale"]["scale-res+"] > 0 and caught["no_swap_negative_scale"]["scale+res+"] == 0
    assert caught["no_swap_negative_resolution"]["scale+res-"] > 0 and caught["no_swap_negative_resolution"]["scale+res+"] == 0
    assert caught["matching_corners"]["scale+res+"] > 0
    assert caught["resolution_before_scale"]["scale-res+"] > 0
    assert caught["domain_on_index"]["scale+res+"] > 0


def test_signs_and_programs_the_corner_tables_cover():
    signs = set()
    for name, spec in rows.CORNER_PROGRAMS.items():
        if name != "two-resolutions":
            signs.add((1 + spec["base"][1] > 0, spec["base"][2] > 0))
            for v in corner_table(name)["params"]:                 # (the solve keeps the signs the table is about)
                assert (1 + v[1] > 0, v[2] > 0) == (1 + spec["base"][1] > 0, spec["base"][2] > 0)
    assert len(signs) == 4
    two = rows.CORNER_PROGRAMS["two-resolutions"]
    assert sum(s["type"] == "resolution_scale" and s["obs"] == rows.BOXED for s in two["systs"]) == 2


def test_restatements_agree_with_the_oracle_on_the_built_tables():
    """reference_bins -- what everything above is held to -- gives the oracle's histogram on the built rows."""
    for t, params in ((threshold_table("c3-shift"), threshold_table("c3-shift")["params"][7]),
                      (threshold_table("scale-negative"), threshold_table("scale-negative")["params"][100]),
                      (corner_table("scale-res-"), corner_table("scale-res-")["params"][5])):
        lo, hi, nb = t["spec"]["geom"]
        geom = oracle.HistGeometry(lo, hi, nb)
        bins, norm = oracle.bin_samples(geom, t["tab"], rows.NFIELDS, t["spec"]["systs"], np.asarray(params, np.float64))
        idx, ind, _ = model.reference_bins(t["tab"], t["spec"]["systs"], params, lo, hi, nb)
        flat = np.zeros(t["tab"].shape[0], np.int64)
        for k in range(len(nb)):
            flat += idx[k] * int(geom.bin_stride[k])
        ok = ind & (flat >= 0) & (flat < geom.total_nbins)
        mine = np.bincount(flat[ok], minlength=geom.total_nbins).astype(np.uint32)
        assert int(ind.sum()) == norm and np.array_equal(mine, bins), t["name"]
