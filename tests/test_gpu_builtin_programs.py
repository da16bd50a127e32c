"""GPU parity, slot by slot: every fill kernel built into the library (pdfz_kernels.hip: the static, ordered and boxed
programs) is reached through the planner's own switches, named by LaunchInfo() and compared bit for bit with the oracle.

The lists below mirror the built-in tables.  A program is written in SLOTS (the columns its launch loads): the
observables the fill bins, then the fields it only reads, then -- ordered and boxed forms -- the observable that is a
constant per granule.  A static program serves two kinds of table:
  * rows / pre-binned: the evaluator has the program's observables (the ones no systematic writes are what the
    pre-binned column replaces) and its extra fields, slot = field;
  * bucketed: the evaluator has one more observable that nothing writes, placed last; the buckets are its bins and the
    compacted problem left to the fill is the program's.

Every case is one group of two members, 20 011 and 5 samples (neither a multiple of 4 or 256), values in -0.1 .. 1.1
over a domain of 0 .. 1.  Nothing is left out: every launcher of every entry is reachable at these sizes (bucketing
accepts a table while its granules are at most 1.3 x rows + 16384 slots, i.e. up to ~80 buckets here; the ordered and
boxed forms are forced)."""
import re

import numpy as np
import pytest

from sxmc_amd import nll, pdfz
from sxmc_amd.capi import DeviceArray
from sxmc_amd.mcmc import make_systematic
from tests.test_gpu_pdfz import assert_same_bits, oracle_eval

pytestmark = pytest.mark.gpu

LDS_MAX_BINS = 40832
SIZES = (20011, 5)
_rng = np.random.default_rng(20011)
TABLES = [_rng.uniform(-0.1, 1.1, size=(n, 8)).astype(np.float32) for n in SIZES]      # shared, never written
POINTS = np.concatenate([_rng.uniform(-0.1, 1.1, size=(97, 5)).astype(np.float32),
                         _rng.integers(0, 2, size=(97, 1)).astype(np.float32)], axis=1)

SHIFT, SCALE, CTSC, RES = "shift", "scale", "ctscale", "resolution_scale"
PARAM = {SHIFT: 0.03, SCALE: -0.02, CTSC: 0.04, RES: 0.1}


def THREE(t):
    return (SHIFT, 1), (SCALE, 0), (RES, 0, t)   # BASELINE configs 3 and 5


# The entries of kPrograms for rows, pre-binned and bucketed tables: (nobs, nslot, ops, launchers).  "pre": LDS histogram
# over a 1- and a 2-byte pre-binned column; "g": histogram beyond LDS, rows and both pre-binned columns; "gran": bucketed
# table, histogram in LDS, beyond LDS, and the sparse runs.  Every entry has the LDS-histogram kernel over rows.
STATIC = [
    (1, 1, (), "pre"), (2, 2, (), "pre"), (3, 3, (), "pre"),
    (1, 1, ((SHIFT, 0),), "gran"), (1, 1, ((SCALE, 0),), "gran"), (1, 1, ((CTSC, 0),), "gran"),
    (1, 1, ((SHIFT, 0), (SCALE, 0)), "gran"), (1, 2, ((RES, 0, 1),), "gran"),
    (1, 2, ((SCALE, 0), (RES, 0, 1)), "gran"), (1, 2, ((SHIFT, 0), (SCALE, 0), (RES, 0, 1)), "gran"),
    (2, 2, ((SHIFT, 0),), "pre"), (2, 2, ((SCALE, 0),), "pre"), (2, 2, ((SHIFT, 1),), "pre"),
    (2, 3, ((SCALE, 0), (RES, 0, 2)), "pre"),
    (2, 3, THREE(2), "gran"),
    (3, 3, ((SHIFT, 0),), "pre"), (3, 3, ((SCALE, 0),), "pre"), (3, 4, ((RES, 0, 3),), "pre"),
    (3, 4, ((SCALE, 0), (RES, 0, 3)), "pre"),
    (3, 4, THREE(3), "pre g"),
    (5, 6, THREE(5), "pre g"),
]
# Its ordered and boxed entries, as the evaluators whose compacted problem they are: (name, table, nobs, nfields,
# systematics by field).  One shifted / scaled observable beside an untouched one: nothing is binned per sample, slot 0 is
# the ordered observable.  The C3 evaluator (e, r, c, e_true): ordered, e is binned per sample (slot 0), e_true is slot 1
# and r the ordered slot 2 -- SHIFT(2), SCALE(0), RES(0, 1); boxed, r is slot 0 and e the boxed slot 2 -- SHIFT(0),
# SCALE(2), RES(2, 1).
C3 = ((SHIFT, 1), (SCALE, 0), (RES, 0, 3))
SORTED = [
    ("ordered(0,1,shift)", "ordered", 2, 2, ((SHIFT, 0),)),
    ("ordered(0,1,scale)", "ordered", 2, 2, ((SCALE, 0),)),
    ("ordered(1,3,c3)", "ordered", 3, 4, C3),
    ("boxed(1,3,c3)", "boxed", 3, 4, C3),
]

SMALL = [6, 5, 4, 3, 2]


def prebin_bound(nbins, written):
    """Largest value of the pre-binned column (sxmc_plan.h, prebin_columns): below 255 it is 1 byte wide, else 2."""
    stride = [int(np.prod(nbins[k + 1:])) for k in range(len(nbins))]
    return sum(nbins[k] * stride[k] for k in range(len(nbins)) if k not in written)


def static_cases():
    out = []
    for nobs, nslot, ops, has in STATIC:
        has = has.split()
        name = "static(%d,%d,%s)" % (nobs, nslot, "+".join(o[0] + str(o[1]) for o in ops) or "none")
        written = {o[1] for o in ops}
        untouched = [k for k in range(nobs) if k not in written]
        rows = dict(nobs=nobs, nfields=nslot, ops=ops)
        out.append((name + "-rows", dict(rows, nbins=SMALL[:nobs], table="rows", hist="lds")))
        if "pre" in has:
            two = SMALL[:nobs]
            two[untouched[-1]] = 40 if nobs == 5 else 300
            for width, nbins in ((1, SMALL[:nobs]), (2, two)):
                assert (prebin_bound(nbins, written) < 255) == (width == 1) and prebin_bound(nbins, written) < 65535
                assert int(np.prod(nbins)) <= LDS_MAX_BINS
                out.append((name + "-pre%d" % width, dict(rows, nbins=nbins, table="prebinned", hist="lds", pre=width)))
        if "g" in has:
            one, two = SMALL[:nobs], SMALL[:nobs]
            one[0] = one[1] = 120
            two[0] = two[1] = 20
            two[untouched[-1]] = 40 if nobs == 5 else 300
            for width, nbins in ((0, one), (1, one), (2, two)):
                assert width == 0 or (prebin_bound(nbins, written) < 255) == (width == 1)
                assert int(np.prod(nbins)) > LDS_MAX_BINS
                out.append((name + ("-global-pre%d" % width if width else "-global-rows"),
                            dict(rows, nbins=nbins, table="prebinned" if width else "rows", hist="global", pre=width,
                                 points=False)))
        if "gran" in has:
            # one more observable, untouched, last: fields shift up by one behind it
            bops = tuple((o[0], o[1]) + tuple(t + 1 for t in o[2:]) for o in ops)
            b = dict(nobs=nobs + 1, nfields=nslot + 1, ops=bops, bucket=True)
            big = ([6000] if nobs == 1 else [300, 40]) + [7]
            assert int(np.prod(big)) > LDS_MAX_BINS
            out.append((name + "-bucketed", dict(b, nbins=SMALL[:nobs] + [7], table="bucketed", hist="lds")))
            out.append((name + "-bucketed-global", dict(b, nbins=big, table="bucketed", hist="global", points=False)))
            out.append((name + "-bucketed-runs", dict(b, nbins=big, table="bucketed+runs(builtin)", hist="global")))
    for name, table, nobs, nfields, ops in SORTED:
        out.append((name, dict(nobs=nobs, nfields=nfields, ops=ops, nbins=SMALL[:nobs], table=table, hist="lds",
                               bucket=True)))
    return out


CASES = static_cases()


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_builtin_program_slot(name, case):
    nobs, nfields, nbins = case["nobs"], case["nfields"], case["nbins"]
    systs = [dict(type=o[0], obs=o[1], pars=[q], **({"true_obs": o[2]} if len(o) > 2 else {}))
             for q, o in enumerate(case["ops"])]
    params = [PARAM[o[0]] for o in case["ops"]] or [0.0]
    points = np.ascontiguousarray(POINTS[:, list(range(nobs)) + [5]]) if case.get("points", True) else None
    E = 0 if points is None else points.shape[0]
    tabs = [np.ascontiguousarray(t[:, :nfields]) for t in TABLES]
    lut = DeviceArray(np.full(max(1, len(tabs) * E), 777.0, np.float32))
    norms = DeviceArray(np.full(len(tabs), 55, np.uint32))
    pbuf = DeviceArray(np.asarray(params, np.float64))
    evs = []
    for j, t in enumerate(tabs):
        ev = pdfz.EvalHist(t, nfields, nobs, [0.0] * nobs, [1.0] * nobs, nbins, dataset=j % 2)
        for s in systs:
            ev.AddSystematic(make_systematic(s))
        if points is not None:
            ev.SetEvalPoints(points)
            ev.SetPDFValueBuffer(lut, j * E, 1)
        ev.SetNormalizationBuffer(norms, j)
        ev.SetParameterBuffer(pbuf, 0, 1)
        evs.append(ev)
    group = nll.EvalGroup(evs)
    group.SetRuntimeKernels(False)                       # a slot without its kernel must not be papered over
    group.SetBucketing(bool(case.get("bucket")))
    group.SetPrebinning(bool(case.get("pre")))
    group.SetOrdering(case["table"] in ("ordered", "boxed"), force=True)
    group.SetBoxes(case["table"] == "boxed")
    group.SetSparse(True)

    info = group.LaunchInfo()
    launches = re.findall(r"^launch \d+: .*$", info, re.M)
    assert launches and "failed" not in info, info
    for line in launches:
        f = dict(kv.split("=", 1) for kv in line.split(": ", 1)[1].split())
        assert f["program"] == "builtin" and f["hist"] == case["hist"], info
        if case["table"] in ("ordered", "boxed"):       # (+codes: the streamed fields as 16-bit codes where there are any)
            assert f["table"] in (case["table"], case["table"] + "+codes"), info
        else:
            assert f["table"] == case["table"], info
    if case["table"] in ("rows", "prebinned"):          # which column is streamed: 4 bytes per float slot, 1 or 2 for the column
        written = {o[1] for o in case["ops"]}
        w = case.get("pre", 0)
        per_row = 4 * (nfields - (nobs - len(written) if w else 0)) + w
        assert group.AlgorithmicBytes()["fill_read"] == per_row * sum(SIZES), info

    group.EvalAsync(points is not None)
    group.EvalFinished()
    got_norms, got_lut = norms.get(), lut.get()
    if case["table"].endswith("+runs(builtin)"):         # (the runs count event bins only: the histogram comes from a dense fill)
        group.EvalAsync(False)
        group.EvalFinished()
        assert np.array_equal(norms.get(), got_norms)
    for j, t in enumerate(tabs):
        o = oracle_eval(t, nfields, [0.0] * nobs, [1.0] * nobs, nbins, systs, params, points=points, dataset=j % 2)
        assert got_norms[j] == o["norm"], (name, j)
        assert np.array_equal(evs[j].GetBins(), o["bins"]), (name, j)
        if points is not None:
            assert_same_bits(got_lut[j * E:(j + 1) * E], o["out"])
    group.close()
    for ev in evs:
        ev.close()
