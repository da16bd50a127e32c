"""CPU: bench.py's command line and its --dump-outputs writer (no GPU: the arrays are made here)."""
import numpy as np
import pytest

import bench


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def test_dump_writes_every_array_as_npy(tmp_path):
    arrays = {"chain": np.arange(12, dtype=np.float32).reshape(4, 3), "nll": np.array([1.5])}
    shapes = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert shapes == {"chain": [4, 3], "nll": [1]}
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_refuses_what_is_not_float32_or_float64(tmp_path):
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), {"counts": np.zeros(3, np.uint32)})


def test_dump_over_the_limit_keeps_a_fixed_sample_with_the_last_row(tmp_path):
    chain = np.arange(1000 * 4, dtype=np.float64).reshape(1000, 4)
    small = np.ones(8, np.float32)
    limit = 100 * 4 * 8 + small.nbytes
    a = bench.dump_outputs(str(tmp_path / "a"), {"chain": chain, "small": small}, limit=limit)
    b = bench.dump_outputs(str(tmp_path / "b"), {"chain": chain, "small": small}, limit=limit)
    assert a == b == {"chain": [100, 4], "small": [8]}
    ca, cb = np.load(tmp_path / "a" / "chain.npy"), np.load(tmp_path / "b" / "chain.npy")
    assert np.array_equal(ca, cb) and np.array_equal(ca[-1], chain[-1])
    assert np.all(np.diff(ca[:, 0]) > 0)                   # rows in their order, none twice
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    total = sum(np.load(tmp_path / "a" / n).nbytes for n in ("chain.npy", "small.npy"))
    assert total <= limit
