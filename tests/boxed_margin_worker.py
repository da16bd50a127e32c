"""Worker of tests/test_gpu_boxed_threshold.py: the boxed fill's bound with its measurement scales, on the GPU.

Run as a child process with SXMC_HIP_LIB = sxmc_amd/csrc/libsxmc_hip_measure.so (only the measurement build can scale
the bound: sxmc_group_set_debug_mode bits 8-23, fill_boxed_body's copy of THE BOUND; bit 4 drops what the queues hold).
Prints one JSON object.

On the threshold tables of tests/boxed_rows.py (rows filling the code cells around every bin edge, the parameter solved
so that an edge sits a few float spacings inside a cell boundary), at the solved parameter vectors:
  * unscaled: misplaced rows (histogram and norm against the oracle's) -- must be 0;
  * the whole threshold scaled by 0.5 and 0.85: misplaced rows, beside the count the CPU model
    (tests/boxed_reference.py) predicts for the same table and vectors -- the negative controls;
  * hook 16: the rows the queues held go missing; what is left was decided by the codes -- the share of built rows;
  * everything but Q scaled by s = 1, 3/4 ... 0: s_min, the smallest s from which upwards nothing is misplaced.
On the corner tables, at each table's base parameters: unscaled misplaced rows, and under hook 16 the share of in-domain
rows counted without the float path (the granules decided from their boxes).
The assertions are the test's; `failures` lists what this worker itself found inconsistent."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle                      # noqa: E402  (the checker)
from sxmc_amd import capi, nll, pdfz           # noqa: E402
from sxmc_amd.capi import DeviceArray          # noqa: E402
from sxmc_amd.mcmc import make_systematic      # noqa: E402
from tests import boxed_reference as model     # noqa: E402
from tests import boxed_rows as rows           # noqa: E402

ROUNDING_SCALES = [1.0, 0.75, 0.5, 0.375, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0]
TOTAL_SCALES = [0.85, 0.5]
THRESHOLD_TABLES = ["c3-shift", "scale-negative"]


class Fill:
    """One table in the boxed form, the oracle beside it."""

    def __init__(self, t):
        spec = t["spec"]
        self.lo, self.hi, self.nb = spec["geom"]
        self.tab, self.systs = t["tab"], spec["systs"]
        self.geom = oracle.HistGeometry(self.lo, self.hi, self.nb)
        self.ev = pdfz.EvalHist(self.tab, rows.NFIELDS, len(self.nb), self.lo, self.hi, self.nb)
        for s in self.systs:
            self.ev.AddSystematic(make_systematic(s))
        self.norm = DeviceArray.zeros(1, np.uint32)
        self.pbuf = DeviceArray(np.asarray(spec["base"], np.float64))
        self.ev.SetNormalizationBuffer(self.norm)
        self.ev.SetParameterBuffer(self.pbuf)
        self.group = nll.EvalGroup([self.ev])
        self.group.SetBoxes(True)
        assert "boxed+codes" in self.group.LaunchInfo(), self.group.LaunchInfo()

    def want(self, params):
        return oracle.bin_samples(self.geom, self.tab, rows.NFIELDS, self.systs, np.asarray(params, np.float64))

    def differences(self, params, want, mode):
        self.pbuf.set(np.asarray(params, np.float64))
        self.group.SetDebugMode(mode)
        self.group.EvalAsync(False)
        self.group.EvalFinished()
        got = self.ev.GetBins()
        return int(np.abs(got.astype(np.int64) - want[0].astype(np.int64)).sum()), int(want[1]) - int(self.norm.get()[0])

    def misplaced(self, params, want, mode):
        """A row in a wrong bin moves one count (two differences), a row wrongly in or out of the domain changes the norm."""
        bins, norm = self.differences(params, want, mode)
        return bins // 2 + abs(norm)

    def missing(self, params, want):
        """Hook 16: the in-domain rows the queues held are counted nowhere -- the norm says how many."""
        return self.differences(params, want, 16)[1]

    def close(self):
        self.group.SetDebugMode(0)
        self.group.close()
        self.ev.close()


def threshold(name, failures):
    t = rows.threshold_table(name)
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    s = spec["streamed"]
    f = Fill(t)
    if f.group.CodesWindows(0) != ([t["base"]], [t["step"]]):
        failures.append("%s: the window is %r, built for %r" % (name, f.group.CodesWindows(0), (t["base"], t["step"])))
    codes = model.encode16(t["tab"][:, s], t["base"], t["step"])
    out = {"name": name, "rows": int(t["tab"].shape[0]), "rows_built": int(t["built"].sum()),
           "parameter_vectors": len(t["params"]), "misplaced_unscaled": 0,
           "misplaced": {str(x): 0 for x in TOTAL_SCALES}, "model_misplaced": {str(x): 0 for x in TOTAL_SCALES},
           "rounding_scale": {str(x): 0 for x in ROUNDING_SCALES}}
    built_in = built_left = model_left = 0
    for i, params in enumerate(t["params"]):
        want = f.want(params)
        out["misplaced_unscaled"] += f.misplaced(params, want, 0)
        if i % 2 == 0:
            # the controls; the model's count for the same rows and vector
            idx_ref, ind, ind_k = model.reference_bins(t["tab"], spec["systs"], params, lo, hi, nb)
            for x in TOTAL_SCALES:
                field, scale = model.dbg_scale(x)
                out["misplaced"][str(x)] += f.misplaced(params, want, field << 16)
                bound = model.streamed_bound(spec["systs"], params, s, t["base"], t["step"], lo[s], hi[s], nb[s],
                                             total_scale=scale)
                idx, trusted, inside, _ = model.classify_codes(codes, bound)
                out["model_misplaced"][str(x)] += int((trusted & ((inside != ind_k[s]) | (inside & (idx != idx_ref[s])))).sum())
            # hook 16: the in-domain rows that go missing were in the queues.  All of them are charged to the built rows
            # (the background's in-domain rows counted as decided): a lower bound on the built rows' share
            missing = f.missing(params, want)
            n_built = int((ind & t["built"]).sum())
            built_in += n_built
            built_left += n_built - missing
            bound = model.streamed_bound(spec["systs"], params, s, t["base"], t["step"], lo[s], hi[s], nb[s])
            model_left += int((ind & t["built"] & ~model.classify_codes(codes, bound)[3]).sum())
        if i % 6 == 0:
            for x in ROUNDING_SCALES:
                out["rounding_scale"][str(x)] += f.misplaced(params, want, model.dbg_scale(x)[0] << 8)
    out["codes_decided_share_of_built_rows"] = built_left / built_in
    out["model_codes_decided_share_of_built_rows"] = model_left / built_in
    f.close()
    return out


def corner(name, failures):
    t = rows.corner_table(name)
    spec = t["spec"]
    lo, hi, nb = spec["geom"]
    f = Fill(t)
    params = spec["base"]
    want = f.want(params)
    groups, boxes = model.layout_granules(t["tab"], rows.BOXED, rows.TRUTH, [spec["unwritten"]], lo, hi, nb)
    out = {"name": name, "rows": int(t["tab"].shape[0]), "in_domain": int(want[1]),
           "misplaced_unscaled": f.misplaced(params, want, 0),
           "model_box_decided_share": model.decided_row_share(t["tab"], groups, boxes, spec["systs"], params, rows.BOXED,
                                                              rows.TRUTH, lo, hi, nb)}
    out["box_decided_share"] = 1.0 - f.missing(params, want) / float(want[1])
    f.close()
    return out


def main():
    if not capi.is_measurement_build():
        raise SystemExit("boxed_margin_worker.py needs SXMC_HIP_LIB = .../libsxmc_hip_measure.so")
    if capi.device_count() < 1:
        raise SystemExit("boxed_margin_worker.py needs a GPU")
    failures = []
    th = [threshold(name, failures) for name in THRESHOLD_TABLES]
    co = [corner(name, failures) for name in rows.CORNER_PROGRAMS]
    s_min = None
    for x in ROUNDING_SCALES:
        if all(t["rounding_scale"][str(x)] == 0 for t in th):
            s_min = x
        else:
            break
    print(json.dumps({"threshold": th, "corner": co, "s_min": s_min, "rounding_scales": ROUNDING_SCALES,
                      "failures": failures}))


if __name__ == "__main__":
    main()
