"""The launch plan, pinned: the full text of sxmc_group_launch_info (table form, kernel, threads, grid, partition, teams,
LDS bytes and the LDS layout word) of a set of small cases equals tests/golden/launch_plans.json line for line.

Results do not depend on the replicas of an LDS histogram or on the size of its queues, so no parity test sees them
change; this one does.  The plans depend on the device (compute units, LDS per CU): the golden records the device it
was made on and every case FAILS on another one -- the project targets one device.  Planning only: one evaluation per
case where the plan is built at first use.

Recording (after a deliberate change of the planner's policy): python -m tests.test_gpu_plan_golden <output.json>"""
import gc
import json
import os
import sys

import numpy as np
import pytest

from sxmc_amd import capi, nll, workloads
from sxmc_amd.mcmc import MCMC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")


def chain(w):
    m = MCMC(w, seed=4, fused=True)
    m.setup(sync_interval=8)
    return m


def close_chain(m):
    for p in m.pdfs:
        p.close()
    m.group.close()


def settle(group, order=True, force=False, boxes=None, codes=None, teams=0, launch=(0, 0)):
    """Every setting the cases vary, each time: a case does not depend on the one before it."""
    group.SetOrdering(order, force=force)
    group.SetBoxes(boxes)
    group.SetCodes(codes)
    group.SetPartitionTeams(teams)
    group.SetLaunchConfig(*launch)
    return group.LaunchInfo()


def plans_config2():
    m = chain(workloads.config2(scale=0.02))
    out = {"c2 prebinned": m.group.LaunchInfo()}
    close_chain(m)
    return out


def plans_config3_small():
    m = chain(workloads.config3(scale=0.01))
    g = m.group
    out = {
        "c3 small, defaults": settle(g),
        "c3 small, ordering forced, no boxes": settle(g, force=True, boxes=False),
        "c3 small, ordering forced, no boxes, no codes": settle(g, force=True, boxes=False, codes=False),
        "c3 small, ordering forced, boxes forced": settle(g, force=True, boxes=True),
        "c3 small, ordering forced, no boxes, 3 teams, 768 x 1": settle(g, force=True, boxes=False, teams=3,
                                                                        launch=(768, 1)),
    }
    close_chain(m)
    return out


def plans_config3_dual():
    m = chain(workloads.config3(scale=0.11))
    out = {}
    for form in (1, 2):
        m.group.SetFillForm(form)
        out["c3 dual plan, fill form %d" % form] = m.group.LaunchInfo()
    close_chain(m)
    return out


def plans_c5_strides():
    """tests/test_gpu_c5_geometry.py's tables with strides below 2^23 (+runs) and reaching it (the note: line)."""
    rng = np.random.default_rng(77)
    lower, upper = [0.0, 0.0, -1.0], [10.0, 6.0, 1.0]
    signals = []
    for j in range(2):
        n = 3_000_001
        e_true = rng.normal(4.0 + j, 1.5, n)
        tab = np.stack([e_true + rng.normal(0, 0.3, n), 6.0 * rng.uniform(size=n) ** (1 / 3), rng.uniform(-1, 1, n),
                        e_true, np.zeros(n)], axis=1).astype(np.float32)
        signals.append(workloads.Signal(tab, 5, nexpected=500.0 + 100 * j, source_id=j))
    ev = workloads._events_from_mixture(rng, signals, 3, 20000, None, None)
    out = {}
    for name, nb in (("c5 geometry, strides below 2^23", [100, 2900, 360]), ("c5 geometry, a stride of 2^23", [100, 2900, 2900])):
        w = workloads.Workload(name, 3, lower, upper, nb, signals, workloads.C3_SYSTS, workloads.C3_SIGMAS, ev, name)
        m = chain(w)
        out[name] = m.group.LaunchInfo()
        close_chain(m)
    return out


def plans_pdfz_group():
    m = chain(workloads.bench_pdfz_group(scale=0.01))
    out = {"bench_pdfz_group, 29 members": m.group.LaunchInfo()}
    close_chain(m)
    return out


def plans_two_coefficients():
    """One member, a three- and a two-coefficient systematic: no built-in program."""
    from tests.test_gpu_pdfz import build_group
    systs = [dict(type="shift", obs=0, pars=[0, 1, 2]), dict(type="scale", obs=1, pars=[3, 0])]
    evs, _, _, _, _ = build_group(np.random.default_rng(31), [90001], 3, [12, 9, 10], systs, [0.02, -0.03, 0.01, 0.05],
                                  nfields=4, lo=-0.1, hi=1.1)
    group = nll.EvalGroup(evs)
    group.SetOrdering(False)
    out = {}
    for rtc in (True, False):
        group.SetRuntimeKernels(rtc)
        out["two coefficients, run-time kernels %s" % ("on" if rtc else "off")] = group.LaunchInfo()
    group.close()
    for e in evs:
        e.close()
    return out


# every builder with the cases it must return: a case that a builder stops returning fails, it does not pass unseen
BUILDERS = {
    plans_config2: ["c2 prebinned"],
    plans_config3_small: ["c3 small, defaults", "c3 small, ordering forced, no boxes",
                          "c3 small, ordering forced, no boxes, no codes", "c3 small, ordering forced, boxes forced",
                          "c3 small, ordering forced, no boxes, 3 teams, 768 x 1"],
    plans_config3_dual: ["c3 dual plan, fill form 1", "c3 dual plan, fill form 2"],
    plans_c5_strides: ["c5 geometry, strides below 2^23", "c5 geometry, a stride of 2^23"],
    plans_pdfz_group: ["bench_pdfz_group, 29 members"],
    plans_two_coefficients: ["two coefficients, run-time kernels on", "two coefficients, run-time kernels off"],
}


def device():
    info = capi.device_info(0)
    return {"compute_units": info["compute_units"], "lds_bytes_per_cu": info["lds_bytes_per_cu"]}


@pytest.fixture(scope="module")
def golden_plans():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("builder", list(BUILDERS), ids=[b.__name__ for b in BUILDERS])
def test_launch_plans_are_the_recorded_ones(golden_plans, builder):
    assert device() == golden_plans["device"], "the golden plans were recorded on another device"
    got = builder()
    # What a builder leaves to Python's cyclic collector goes now.  Left for later, the collector has released it in
    # the middle of a later test's graph recording (tests/test_gpu_step_end.py, config 3 with 40000 events), and a
    # release of device memory inside a recording ends it: "operation failed due to a previous error during capture".
    gc.collect()
    assert sorted(got) == sorted(BUILDERS[builder])
    for name, text in got.items():
        print(name + "\n" + text)
        assert text.splitlines() == golden_plans["plans"][name], name


def test_every_recorded_plan_is_built(golden_plans):
    names = [name for cases in BUILDERS.values() for name in cases]
    assert len(names) == len(set(names)) and set(names) == set(golden_plans["plans"])


if __name__ == "__main__":
    plans = {}
    for b in BUILDERS:
        for name, text in b().items():
            assert name not in plans
            plans[name] = text.splitlines()
    with open(sys.argv[1], "w") as f:
        json.dump({"device": device(), "plans": plans}, f, indent=1)
        f.write("\n")
