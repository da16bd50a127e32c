"""GPU: the BOXED fill on rows built on its bound and on its box corners (fill_boxed_kernel; tests/boxed_rows.py).

Random tables almost never meet the two conditions under which fill_boxed_body could count a row wrongly without
looking at it: a transformed bin edge of the streamed observable a hair inside a code cell's boundary, and a granule
whose box has a corner within ulps of an edge of the boxed observable.  tests/boxed_rows.py builds both and solves the
parameters; tests/test_boxed_model_cpu.py shows on the CPU that a halved threshold and five planted mistakes in the
interval rule do go wrong on exactly these inputs.  Here the PRODUCT library must give the oracle's histograms and
norms, bit for bit, at every solved parameter vector: boxed under partitions 0, 1, 2, with the queues at their smallest,
and in the ordered form.  The measurement build then repeats the threshold tables with the bound scaled
(tests/boxed_margin_worker.py, a child process): nothing misplaced as shipped, the negative controls firing against the
CPU model's predicted counts, the codes- and box-decided shares at their floors, the margin s_min recorded.
Reference arithmetic: bin_samples of the oracle (pdfz.cpp:306-331, 388-398 restated)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sxmc_amd import capi
from tests import boxed_rows as rows
from tests.test_gpu_boxed import evaluate, make_group
from tests.test_gpu_pdfz import oracle_eval

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (boxes, partition, log2 of the queues' entries)
FORMS = [(True, 0, 0), (True, 1, 0), (True, 2, 0), (True, 0, 9), (False, 0, 0)]


def hold_to_the_oracle(t, window=None):
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    tab, systs = t["tab"], spec["systs"]
    want = [oracle_eval(tab, rows.NFIELDS, lo, hi, nb, systs, p) for p in t["params"]]
    group, evs, norms, pbuf = make_group([tab], systs, t["params"][0], lo, hi, nb, rows.NFIELDS)
    bad = []
    for boxes, partition, qlog in FORMS:
        group.SetBoxes(boxes)
        group.SetPartition(partition)
        group.SetCodesQueueLog(qlog)
        info = group.LaunchInfo()
        assert ("boxed+codes" in info) == boxes and (boxes or "boxed" not in info), (t["name"], boxes, partition, qlog, info)
        if boxes and window is not None:
            assert group.CodesWindows(0) == ([window[0]], [window[1]]), "the built rows moved the window"
        for i, params in enumerate(t["params"]):
            pbuf.set(np.asarray(params, np.float64))
            bins, nrm = evaluate(group, evs, norms)
            if not np.array_equal(bins[0], want[i]["bins"]) or nrm[0] != want[i]["norm"]:
                bad.append((boxes, partition, qlog, i, params, t["solved"][i],
                            int(np.abs(bins[0].astype(np.int64) - want[i]["bins"].astype(np.int64)).sum()),
                            int(nrm[0]) - int(want[i]["norm"])))
    group.close()
    for e in evs:
        e.close()
    assert not bad, (t["name"], len(bad), bad[:5])


@pytest.mark.parametrize("name", ["c3-shift", "ctscale-streamed", "two-resolutions", "scale-negative"])
def test_rows_built_on_the_boxed_bound_are_binned_like_the_oracle(name):
    """c3-shift: config 3's program (built in); the others are compiled at run time."""
    t = rows.threshold_table(name)
    nedges = t["spec"]["geom"][2][t["spec"]["streamed"]] + 1
    assert len(t["params"]) >= 36 * (nedges - 1) and int(t["built"].sum()) > 2000 * nedges
    hold_to_the_oracle(t, window=(t["base"], t["step"]))


@pytest.mark.parametrize("name", list(rows.CORNER_PROGRAMS))
def test_granules_with_a_box_corner_on_an_edge_are_binned_like_the_oracle(name):
    t = rows.corner_table(name)
    assert len(t["params"]) >= 150
    hold_to_the_oracle(t)


def test_margin_of_the_boxed_bound_and_negative_controls(tmp_path):
    """The record (boxed_margin.json) is kept in the directory SXMC_RECORD_DIR names, else in the test's own."""
    env = dict(os.environ, SXMC_HIP_LIB=capi.MEASURE_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boxed_margin_worker.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    record_dir = os.environ.get("SXMC_RECORD_DIR") or str(tmp_path)
    os.makedirs(record_dir, exist_ok=True)
    with open(os.path.join(record_dir, "boxed_margin.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print("s_min %r; misplaced at 0.5 / 0.85, model beside: %r" % (rec["s_min"], [
        (t["name"], t["misplaced"], t["model_misplaced"]) for t in rec["threshold"]]))
    assert rec["failures"] == [], rec["failures"]
    for t in rec["threshold"]:
        # the bound as shipped: nothing misplaced
        assert t["misplaced_unscaled"] == 0 and t["rounding_scale"]["1.0"] == 0, t
        # NEGATIVE CONTROLS, the expectation from the CPU model on the same table: a threshold half as large as the bound
        # misplaces at least half of what the model predicts (rows in granules that took the float path are binned
        # exactly and lower the count), one at 85 % misplaces rows
        assert t["model_misplaced"]["0.5"] > 1000, t
        assert t["misplaced"]["0.5"] >= 0.5 * t["model_misplaced"]["0.5"], t
        assert t["model_misplaced"]["0.85"] > 0 and t["misplaced"]["0.85"] > 0, t
        # the codes decided the built rows (hook 16 drops what the queues hold)
        assert t["codes_decided_share_of_built_rows"] > rows.TRUSTED_FLOOR[t["name"]], t
    for c in rec["corner"]:
        assert c["misplaced_unscaled"] == 0, c
        assert c["box_decided_share"] > rows.DECIDED_FLOOR[c["name"]], c
    # s_min is RECORDED, not asserted to be below 1: with one field the roundings' share may not be able to show
    assert "s_min" in rec
