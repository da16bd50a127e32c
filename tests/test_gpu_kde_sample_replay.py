"""GPU: sxmc_kde_random_sample (kde_flag / scan / kde_scatter and kde_sample_kernel<D, ADAPT>, sxmc_kde_draw.cpp) held
to the numpy replay of tests/kde_sample_reference.py draw by draw.

For every case ev.RandomSample(...) against draw(...) with the evaluator's own bandwidths and local factors: every event
the replay does not flag as ambiguous equal in all D + 1 floats as bytes; an ambiguous coordinate (the replay's xd within
2^-40 max(|xd|, hw) of a float midpoint or of a bound) at most one float step off; events that came near a cut bound
left out; at most 1e-3 of the events excused; ev.SamplePool() equal to the replay's n and to the norm.  Each case prints
its one-step mismatches with the replay's distance to the midpoint in units of 2^-53 max(|xd|, hw).

The cases (tests/kde_sample_reference.cases; tests/test_kde_sample_reference_cpu.py decides on the CPU that each reaches
its path, keeps within the cap, and that the comparison fails on eight planted errors): 1-4 observables under seeds 7,
2^32 + 7 and 2^63 + 12345; compaction at 255, 256, 257 and 70 001 rows with every third row outside the domain; a shift,
a scale and a resolution scale that move rows out of and into the domain; adaptive bandwidths with rows outside the
domain in between, on the evaluator and on a shared one; [0.1, 0.2) under bandwidth scales 0.001, 50 and 1e-6 and
[0.7, 0.8) under 0.001 (the clamps to bottom and top); cuts that keep 30 %; cuts that keep 0.5 %, where the call fails
with the replay's count of exhausted events; 2^20 + 257 events (lanes take a second event).

Measured on an MI355X (gfx950, ROCm's device library), all 26 cases, 3.2 million events compared: no event wrong and NO
one-step mismatch at all, not even among the coordinates the replay flags as ambiguous (between 0 and 3.7e-4 of a case's
events; the cap is 1e-3) -- so there is no largest distance to report, and nothing about the device's erfc / erfcinv to
find against the threshold of 2^-43 max(|xd|, hw) (1024 of the printed units).  The exhaustion case: 187 events on the
device, 187 in the replay, none near a cut bound.  Each case runs in under half a second.  A one-off build of the
library with lambda read at the place in the in-domain list instead of the table row (not committed) fails both adaptive
cases with 99 813 of 100 000 events wrong -- the count the replay's own lam_by_position variant gives on the CPU -- and
passes the fixed-bandwidth ones."""
import re

import numpy as np
import pytest

from sxmc_amd import capi, pdfz
from sxmc_amd.mcmc import make_systematic
from tests import kde_sample_reference as R
from tests.test_gpu_kde import gpu_kde

pytestmark = pytest.mark.gpu

CASES = R.cases()


def evaluated(case):
    """(the evaluator to draw from after an evaluation at the case's parameters, its norm, evaluators to close)."""
    ev = pdfz.EvalKernel(case.table.ravel(), case.nfields, case.D, case.lower, case.upper, case.scale,
                         dataset=case.dataset, bandwidth_sensitivity=case.alpha)
    for s in case.systs:
        ev.AddSystematic(make_systematic(s))
    keep = [ev]
    if case.shared:
        ev = pdfz.EvalKernel.Shared(ev)
        keep.append(ev)
    pts = np.zeros((4, case.D + 1), np.float32)
    pts[:, :case.D] = (np.asarray(case.lower) + np.asarray(case.upper)) / 2
    pts[:, case.D] = case.dataset
    got = gpu_kde(None, None, case.D, case.lower, case.upper, None, case.systs, case.params, pts.ravel(), ev=ev)
    return ev, got["norm"], keep


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_replay(name):
    case = CASES[name]
    ev, norm, keep = evaluated(case)
    h, lam = ev.Bandwidths(), ev.LocalFactors()
    assert np.all(lam == 1.0) == (case.alpha == 0.0)
    d, n = case.replay(h, lam)
    R.check_replay(case, d, n)
    assert ev.SamplePool() == n == norm
    lo, hi = case.cuts if case.cuts else (None, None)
    if d["exhausted"]:
        with pytest.raises(capi.SxmcError) as err:
            ev.RandomSample(case.nevents, case.seed, lowers=lo, uppers=hi)
        m = re.search(r"(\d+) of %d events" % case.nevents, str(err.value))
        assert m, str(err.value)
        near = int(d["at_cut"].sum())
        print("%s: the device exhausted %s events, the replay %d (%d came near a cut bound)"
              % (name, m.group(1), d["exhausted"], near))
        assert abs(int(m.group(1)) - d["exhausted"]) <= near
    else:
        got = ev.RandomSample(case.nevents, case.seed, lowers=lo, uppers=hi)
        res = R.compare(got, d, name)
        print("%s: largest distance of a one-step mismatch %s (a finding above 2^10 = 1024)" % (name, res["largest"]))
        assert res["excused"] <= 1e-3
        assert res["wrong"] == 0
    for e in keep[::-1]:
        e.close()
