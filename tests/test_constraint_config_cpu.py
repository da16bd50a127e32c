"""CPU: the fit configuration's key "constraint_correlations" -- groups of named parameters with a correlation matrix
each -- read alike by sxmc_amd/io.py and sxmc::load_config (config.h, through tests/cpp/constraint_config_dump) into the
same P x P matrix, with the same message for every refusal; and a configuration without the key loads exactly as it did
before the key existed (tests/golden/constraint_config_before.json: both loaders' dumps, recorded from the commit before).

The fit is tests/test_io_cpu.py's EXAMPLE: parameters sig_a (no constraint), shared (0.25), energy_scale_0 (0.01),
energy_resolution_0 (0.001), energy_resolution_1 (no constraint)."""
import json
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import io
from tests.test_io_cpu import DUMP, EXAMPLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NAMES = ["sig_a", "shared", "energy_scale_0", "energy_resolution_0", "energy_resolution_1"]


@pytest.fixture(scope="module")
def dump():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "constraints.mk", "constraint_config_dump"])
    return os.path.join(CPP, "constraint_config_dump")


def text_with(groups):
    root = json.loads(io.strip_comments(EXAMPLE))
    if groups is not None:
        root["fit"]["constraint_correlations"] = groups
    return json.dumps(root)


def both(tmp_path, text, exe):
    """(python result, C++ result): each the matrix as a list of rows (None without the key), or ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = None if fc.constraint_correlation is None else fc.constraint_correlation.tolist()
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        flat = json.loads(r.stdout)["rho"]
        cpp = None if flat is None else np.array(flat, np.float64).reshape(len(NAMES), len(NAMES)).tolist()
    else:
        assert r.returncode == 1 and r.stderr.startswith("constraint_config_dump: "), r.stderr
        cpp = ("error", r.stderr[len("constraint_config_dump: "):].strip())
    return py, cpp


def group(parameters, matrix):
    return {"parameters": parameters, "matrix": matrix}


def test_groups_are_scattered_into_the_same_matrix(tmp_path, dump):
    assert both(tmp_path, text_with(None), dump) == (None, None)                       # absent: as before
    py, cpp = both(tmp_path, text_with([]), dump)
    assert py == cpp == np.eye(5).tolist()
    py, cpp = both(tmp_path, text_with([group(["energy_scale_0", "energy_resolution_0"], [[1, -0.6], [-0.6, 1]])]), dump)
    want = np.eye(5)
    want[2, 3] = want[3, 2] = -0.6
    assert py == cpp == want.tolist()
    # two disjoint groups, names in another order than the vector's; a group of one
    py, cpp = both(tmp_path, text_with([group(["energy_resolution_0", "shared"], [[1, 0.25], [0.25, 1]]),
                                        group(["energy_scale_0"], [[1]]), group(["sig_a"], [[1.0]])]), dump)
    want = np.eye(5)
    want[3, 1] = want[1, 3] = 0.25
    assert py == cpp == want.tolist()
    py, cpp = both(tmp_path, text_with([group(["energy_resolution_0", "shared", "energy_scale_0"],
                                              [[1, 0.25, -0.5], [0.25, 1, 0.125], [-0.5, 0.125, 1]])]), dump)
    want = np.eye(5)
    idx = [3, 1, 2]
    want[np.ix_(idx, idx)] = [[1, 0.25, -0.5], [0.25, 1, 0.125], [-0.5, 0.125, 1]]
    assert py == cpp == want.tolist()


PAIR = ["energy_scale_0", "energy_resolution_0"]


@pytest.mark.parametrize("groups,message", [
    ([group(["energy_scale_0", "energy_res_0"], [[1, 0.5], [0.5, 1]])],
     'fit: constraint_correlations[0]: unknown parameter "energy_res_0"'),
    ([group(["likelihood", "shared"], [[1, 0.5], [0.5, 1]])],
     'fit: constraint_correlations[0]: unknown parameter "likelihood"'),
    ([group(PAIR, [[1, 0.5], [0.5, 1]]), group(["shared", "energy_scale_0"], [[1, 0.5], [0.5, 1]])],
     'fit: constraint_correlations[1]: parameter "energy_scale_0" is already in a group'),
    ([group(["shared", "shared"], [[1, 0.5], [0.5, 1]])],
     'fit: constraint_correlations[0]: parameter "shared" is already in a group'),
    ([group(PAIR, [[1, 0.5, 0], [0.5, 1, 0], [0, 0, 1]])],
     'fit: constraint_correlations[0]: "matrix" must be 2 x 2 for its 2 parameters'),
    ([group(PAIR, [[1, 0.5], [0.5]])], 'fit: constraint_correlations[0]: "matrix" must be 2 x 2 for its 2 parameters'),
    ([group(PAIR, [1, 0.5, 0.5, 1])], 'fit: constraint_correlations[0]: "matrix" must be 2 x 2 for its 2 parameters'),
    ([group(PAIR, [[1, 0.5], [0.4, 1]])], "fit: constraint_correlations: constraint correlation: not symmetric at (3, 2)"),
    ([group(PAIR, [[1, 1], [1, 1]])],
     "fit: constraint_correlations: constraint correlation: not positive definite at parameter 3"),
    ([group(PAIR + ["shared"], [[1, .9, -.9], [.9, 1, .9], [-.9, .9, 1]])],
     "fit: constraint_correlations: constraint correlation: not positive definite at parameter 3"),
    ([group(PAIR, [[0.5, 0.1], [0.1, 1]])],
     "fit: constraint_correlations: constraint correlation: diagonal entry (2, 2) is not 1"),
    ([group(PAIR, [[1, 1.5], [1.5, 1]])],
     "fit: constraint_correlations: constraint correlation: entry (2, 3) is not a finite number in [-1, 1]"),
    ([group(["energy_scale_0", "energy_resolution_1"], [[1, 0.5], [0.5, 1]])],
     "fit: constraint_correlations: constraint correlation: parameter 4 has no constraint (sigma <= 0) but entry (4, 2) "
     "is not 0"),
    ([group(["sig_a", "shared"], [[1, 0.5], [0.5, 1]])],
     "fit: constraint_correlations: constraint correlation: parameter 0 has no constraint (sigma <= 0) but entry (0, 1) "
     "is not 0"),
    ([group(PAIR, [[1, "x"], ["x", 1]])], "matrix[][]: not a number"),
    ([group([1, 2], [[1, 0], [0, 1]])], "parameters[]: not a string"),
    ([{"parameters": PAIR}], 'fit: constraint_correlations[0]: a group is {"parameters": [names], "matrix": [[...]]}'),
    (["energy_scale_0"], 'fit: constraint_correlations[0]: a group is {"parameters": [names], "matrix": [[...]]}'),
    ({"parameters": PAIR, "matrix": [[1, 0], [0, 1]]}, 'fit: "constraint_correlations" is not a list of groups'),
])
def test_refused_with_the_same_message(tmp_path, dump, groups, message):
    py, cpp = both(tmp_path, text_with(groups), dump)
    assert py == cpp == ("error", message)


def python_dump(fc):
    def plain(v):
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, np.ndarray):
            return plain(v.tolist())
        if isinstance(v, (np.floating, float)):
            return repr(float(v))
        if isinstance(v, np.integer):
            return int(v)
        return v
    return {k: plain(v) for k, v in sorted(vars(fc).items()) if k not in ("constraint_correlation", "base_dir")}


def test_a_configuration_without_the_key_loads_as_it_did_before(tmp_path):
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "constraint_config_before.json")))
    fc = io.load_config(EXAMPLE)
    assert fc.constraint_correlation is None
    assert json.loads(json.dumps(python_dump(fc))) == before["load_config"]
    subprocess.check_call(["make", "-s", "-C", CPP, "config_dump"])
    good = dict(energy=np.linspace(5, 15, 64).astype(np.float32), radius=np.linspace(0, 12, 64), mc_energy=np.arange(64))
    np.savez(tmp_path / "a.npz", **good)
    np.savez(tmp_path / "b.npz", **good)
    (tmp_path / "fit.json").write_text(text_with(None))
    r = subprocess.run([DUMP, str(tmp_path / "fit.json")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout == before["config_dump"]
