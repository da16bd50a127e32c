"""GPU: two paths of the weighted histogram fill that tests/test_gpu_weighted_fill.py does not reach, with that file's
Evaluator, reference and same_bits -- as BYTES against the oracle on the table with row i repeated m_i times:
the shape-agnostic weighted kernel counting straight into HBM, and several weighted members through one workgroup's
list of segments.  No tolerance anywhere."""
import numpy as np
import pytest

from sxmc_amd import nll
from tests.test_gpu_weighted_fill import (LDS_MAX_BINS, SHAPES, Evaluator, _launch_info, eval_points, make_table,
                                          reference, same_bits)

pytestmark = pytest.mark.gpu

GENERIC_BEYOND_LDS_NBINS = [8, 8, 8, 8, 10]   # 40 960 bins > LDS_MAX_BINS = 40 832


def generic_beyond_lds_case(with_points):
    """Inputs and oracle result of test_generic_kernel_with_its_histogram_beyond_lds (no GPU needed)."""
    nfields, systs, params = SHAPES[5]
    rng = np.random.default_rng(55 + int(with_points))
    table = make_table(rng, 257, nfields)
    m = rng.integers(0, 4, size=257).astype(np.uint32)
    points = eval_points(rng, 120, 5) if with_points else None
    want = reference(table, nfields, GENERIC_BEYOND_LDS_NBINS, systs, params, m, points)
    return table, m, points, want


@pytest.mark.parametrize("with_points", [False, True])
def test_generic_kernel_with_its_histogram_beyond_lds(with_points):
    """The shape-agnostic weighted kernel (nslot = 8) counting straight into HBM: a histogram just too large for LDS."""
    assert int(np.prod(GENERIC_BEYOND_LDS_NBINS)) > LDS_MAX_BINS
    nfields, systs, params = SHAPES[5]
    table, m, points, want = generic_beyond_lds_case(with_points)
    assert want["norm"] > 0 and int(want["bins"].sum()) > 0
    e = Evaluator(table, nfields, GENERIC_BEYOND_LDS_NBINS, systs, params, m, points)
    got = e.run()
    info = _launch_info(e.ev)
    assert "program=generic+weighted" in info and "hist=global" in info and "table=rows" in info, info
    assert same_bits(got["bins"], want["bins"]) and got["norm"] == want["norm"]
    if with_points:
        assert same_bits(got["out"], want["out"])
    again = e.run()
    assert same_bits(again["bins"], got["bins"]) and again["norm"] == got["norm"] and same_bits(again["out"], got["out"])
    e.close()


SLICED_ROWS = (5, 64, 255, 256, 257, 300)
SLICED_NBINS = ([5, 6, 7], [7, 6, 5], [5, 6, 7], [1, 1, 1], [5, 6, 7], [7, 6, 5])


def sliced_members_case():
    """Tables, multiplicities, evaluation points and oracle results of test_weighted_members_through_one_segment_list."""
    nfields, systs, params = SHAPES["c3"]
    rng = np.random.default_rng(66)
    tables = [make_table(rng, n, nfields) for n in SLICED_ROWS]
    mult = [rng.integers(0, 4, size=n).astype(np.uint32) for n in SLICED_ROWS]
    # (the 5-row member: three rows well inside the domain, each counted, so that its in-domain total is not 0)
    tables[0][2:] = rng.uniform(0.2, 0.8, size=(3, nfields)).astype(np.float32)
    mult[0][2:] = [1, 2, 3]
    points = eval_points(rng, 60, 3)
    want = [reference(t, nfields, nb, systs, params, m, points) for t, m, nb in zip(tables, mult, SLICED_NBINS)]
    return tables, mult, points, want


def test_weighted_members_through_one_segment_list():
    """Six weighted members of config 3's program, 5 to 300 rows and different histograms, at 64 lanes per workgroup: 286
    units sliced over 5 workgroups, so a workgroup's list of segments spans members (the first one's: all of member 0,
    all of member 1, the start of member 2) -- the LDS histogram cleared between members of different size, the
    workgroup's in-domain total reset per member."""
    nfields, systs, params = SHAPES["c3"]
    tables, mult, points, want = sliced_members_case()
    assert all(w["norm"] > 0 for w in want)
    evs = [Evaluator(t, nfields, nb, systs, params, m, points) for t, m, nb in zip(tables, mult, SLICED_NBINS)]
    g = nll.EvalGroup([e.ev for e in evs])
    g.SetLaunchConfig(64, 1)
    for do_eval_pdf in (True, False, True):
        g.EvalAsync(do_eval_pdf)
        g.EvalFinished()
        for i, (e, w) in enumerate(zip(evs, want)):
            got = e.result()
            assert same_bits(got["bins"], w["bins"]) and got["norm"] == w["norm"], (i, do_eval_pdf)
            assert same_bits(got["out"], w["out"]), (i, do_eval_pdf)
    launches = [line for line in g.LaunchInfo().splitlines() if line.startswith("launch")]
    assert len(launches) == 1 and "program=builtin+weighted" in launches[0] and "members=6" in launches[0], launches
    assert "hist=lds" in launches[0] and "threads=64 grid=5 partition=1 " in launches[0], launches
    for e in evs:
        e.close()
    g.close()
