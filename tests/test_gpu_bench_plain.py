"""GPU box: a plain `python bench.py` run is lean -- set-up, warm-up, the timed steps, the line -- and
`--dump-outputs DIR` writes what the timed steps computed, the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plain_run(tmp_path, tag, steps):
    out = tmp_path / tag
    env = dict(os.environ, SXMC_BENCH_FULL=str(tmp_path / (tag + "_full.json")))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "5", "--prewarm", "20", "--scale", "0.02", "--events", "5000",
                        "--dump-outputs", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [x for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    steps = 37                                      # (not a multiple of the 10 steps a graph replays)
    line, out = plain_run(tmp_path, "a", steps)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-2     # one GPU: value = steps / elapsed
    # what --full measures beside the headline is not measured by a plain run
    assert line["roofline"] is None and line["parity"] is None and line["cpu_baseline"] is None
    assert line["experiments"] is None and line["also"] is None
    names = sorted(p.name for p in out.iterdir())
    assert names == ["accepted.npy", "chain.npy", "current_nll.npy", "current_vector.npy", "proposed_nll.npy",
                     "proposed_vector.npy"]
    first = {n: np.load(out / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in first.values())
    assert sum(a.nbytes for a in first.values()) <= 64 << 20
    chain = first["chain.npy"]
    npar = first["current_vector.npy"].size
    assert chain.shape == (steps, npar + 1)                 # one row per timed step
    # the last row is where the chain stands after the last step: its vector and NLL (float32 in the row)
    assert np.array_equal(chain[-1, :npar], first["current_vector.npy"].astype(np.float32))
    assert chain[-1, -1] == np.float32(first["current_nll.npy"][0])
    _, again = plain_run(tmp_path, "b", steps)
    for n in names:
        assert np.array_equal(np.load(again / n), first[n]), n


@pytest.mark.gpu
def test_plain_two_rank_run_over_gloo_prints_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["SXMC_DIST_BACKEND"] = "gloo"
    env["SXMC_BENCH_FULL"] = str(tmp_path / "full.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                        "--prewarm", "20", "--scale", "0.02", "--events", "5000", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [x for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["parity"] is None and line["experiments"] is None and line["collective"] is None
    assert np.load(tmp_path / "d" / "chain.npy").shape[0] == 20          # rank 0's chain
