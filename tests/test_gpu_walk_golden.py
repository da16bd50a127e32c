"""Whole walks of the C++ driver (sxmc::MCMC, sxmc_amd/include/sxmc/mcmc.h), pinned: tests/cpp/walk_dump.cpp walks the
small fit of the C++ tests in every form -- sequential, graph-replayed, look-ahead, not consuming, the reference's
launches, with the lookup table, debug mode from an empty chain, on a caller's stream, in lockstep sets, in
concurrent lanes and over two logical ranks of the multi-GPU runner -- and each case's line (rows, accepted steps, a hash of the rows, first and last row as float bits;
intervals per experiment) equals tests/golden/walk_chains.json.

The other walk tests compare the forms with each other, so a change that moved all of them together would pass them;
this one does not.  The golden records the device it was made on and every case FAILS on another one.

Recording (after a deliberate change of what a walk computes): python -m tests.test_gpu_walk_golden <output.json>"""
import json
import os
import subprocess
import sys

import pytest

from sxmc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "walk_chains.json")

CASES = [
    "default",
    "graph_steps 8",
    "lookahead, graph_steps 0",
    "lookahead, graph_steps 6",
    "consume off",
    "reference_form",
    "lut_output",
    "debug_mode, 40 steps, no burn-in, sync_interval 16",
    "caller's non-blocking stream, graph_steps 8",
    "ensemble_lockstep, 2 chains in 1 set, graph_steps 8",
    "ensemble_concurrent, 2 lanes, graph_steps 8",
    "ensemble_concurrent, projection intervals, 2 lanes, graph_steps 8",
    "ensemble_multi_gpu, host staging, 2 ranks on device 0, lockstep 2x1",
    "ensemble_multi_gpu, host staging, 2 ranks on device 0, concurrent 2",
]


def device():
    return {"compute_units": capi.device_info(0)["compute_units"]}


def dump():
    """One run of the dump program: {case name: the rest of its line}."""
    subprocess.check_call(["make", "-s", "-C", CPP, "walk_dump"])
    r = subprocess.run([os.path.join(CPP, "walk_dump")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [line.split("\t", 1) for line in r.stdout.splitlines() if "\t" in line]
    assert len(lines) == len({name for name, _ in lines}), "a case was printed twice"
    return dict(lines)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def walked():
    return dump()


@pytest.mark.parametrize("case", CASES)
def test_walk_is_the_recorded_one(golden, walked, case):
    assert device() == golden["device"], "the golden chains were recorded on another device"
    assert case in walked, "walk_dump did not print this case"
    print(case + "\n" + walked[case])
    assert walked[case] == golden["cases"][case]


def test_every_recorded_walk_is_walked(golden, walked):
    assert set(golden["cases"]) == set(CASES) and set(walked) == set(CASES)
    # what the lines say beyond the chains: the look-ahead walk needs fewer passes than steps, and the lockstep sets and
    # the concurrent lanes give the intervals of the one-at-a-time loop
    for case in CASES:
        if case.startswith("lookahead"):
            assert walked[case].endswith(" passes<333 1")
        if case.startswith("ensemble"):
            assert walked[case].endswith(" =ensemble 1")


if __name__ == "__main__":
    cases = dump()
    assert sorted(cases) == sorted(CASES), sorted(cases)
    with open(sys.argv[1], "w") as f:
        json.dump({"device": device(), "cases": {name: cases[name] for name in CASES}}, f, indent=1)
        f.write("\n")
