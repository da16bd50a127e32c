"""CPU: the fit configuration's keys "proposal" ("diagonal" | "covariance") and "proposal_shrinkage" (a number in
(0, 1]), read alike by sxmc_amd/io.py and sxmc::load_config (config.h, through a dump driver built here) with the same
message for every refusal; and a configuration without the keys loads exactly as before."""
import json
import subprocess

import pytest

from sxmc_amd import io
from tests.test_kde_sample_cpu import build_cpp, config_text


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_cpp(tmp_path_factory.mktemp("fit_proposal_dump"), "fit_proposal_dump")


def text_with(**fit_keys):
    root = json.loads(config_text())
    root["fit"].update(fit_keys)
    return json.dumps(root)


def both(tmp_path, text, exe):
    """(python result, C++ result): each (proposal, shrinkage), or ("error", message)."""
    path = tmp_path / "fit.json"
    path.write_text(text)
    try:
        fc = io.load_config(str(path))
        py = (fc.proposal, float(fc.proposal_shrinkage))
    except ValueError as e:
        py = ("error", str(e))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    if r.returncode == 0:
        d = json.loads(r.stdout)
        cpp = (d["proposal"], float(d["proposal_shrinkage"]))
    else:
        assert r.returncode == 1 and r.stderr.startswith("fit_proposal_dump: "), r.stderr
        cpp = ("error", r.stderr[len("fit_proposal_dump: "):].strip())
    return py, cpp


def test_keys_accepted_and_defaulted(tmp_path, dump):
    assert both(tmp_path, config_text(), dump) == (("diagonal", 0.05), ("diagonal", 0.05))     # absent: as before
    assert both(tmp_path, text_with(proposal="diagonal"), dump) == (("diagonal", 0.05), ("diagonal", 0.05))
    assert both(tmp_path, text_with(proposal="covariance"), dump) == (("covariance", 0.05), ("covariance", 0.05))
    for v in (1, 1.0, 0.5, 0.05, 1e-300, 0.9999999999999999):
        py, cpp = both(tmp_path, text_with(proposal="covariance", proposal_shrinkage=v), dump)
        assert py == cpp == ("covariance", float(v))


SHRINKAGE_RANGE = 'fit: "proposal_shrinkage" must be a number in (0, 1]'
SHRINKAGE_ALONE = 'fit: "proposal_shrinkage" is only for "proposal": "covariance"'


@pytest.mark.parametrize("keys,message", [
    (dict(proposal="haario"), 'fit: unknown "proposal" "haario" ("diagonal" or "covariance")'),
    (dict(proposal="Covariance"), 'fit: unknown "proposal" "Covariance" ("diagonal" or "covariance")'),
    (dict(proposal=""), 'fit: unknown "proposal" "" ("diagonal" or "covariance")'),
    (dict(proposal=1), "proposal: not a string"),
    (dict(proposal=["covariance"]), "proposal: not a string"),
    (dict(proposal_shrinkage=0.05), SHRINKAGE_ALONE),
    (dict(proposal="diagonal", proposal_shrinkage=0.05), SHRINKAGE_ALONE),
    (dict(proposal="covariance", proposal_shrinkage=0), SHRINKAGE_RANGE),
    (dict(proposal="covariance", proposal_shrinkage=-0.05), SHRINKAGE_RANGE),
    (dict(proposal="covariance", proposal_shrinkage=1.0000000000000002), SHRINKAGE_RANGE),
    (dict(proposal="covariance", proposal_shrinkage=2), SHRINKAGE_RANGE),
    (dict(proposal="covariance", proposal_shrinkage="1e999"), None),
    (dict(proposal="covariance", proposal_shrinkage="0.05"), "proposal_shrinkage: not a number"),
    (dict(proposal="covariance", proposal_shrinkage=[0.05]), "proposal_shrinkage: not a number"),
])
def test_keys_refused_with_the_same_message(tmp_path, dump, keys, message):
    text = text_with(**keys)
    if message is None:      # a number that overflows to infinity in both parsers
        text = text.replace('"1e999"', "1e999")
        message = SHRINKAGE_RANGE
    py, cpp = both(tmp_path, text, dump)
    assert py == cpp == ("error", message)


def test_fit_proposal_alone():
    assert io.fit_proposal({}) == ("diagonal", 0.05)
    assert io.fit_proposal({"proposal": "covariance", "proposal_shrinkage": 0.25}) == ("covariance", 0.25)
