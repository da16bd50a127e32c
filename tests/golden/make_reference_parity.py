#!/usr/bin/env python3
"""Records tests/golden/reference_parity.json: what the fitted code's own compiled CPU-mode translation units compute
on the cases of tests/reference_cases.py.

    python -m tests.golden.make_reference_parity [OUT.json]

needs oracle/_ref/ref_driver and oracle/_ref/ref_driver_san (oracle/ref/Makefile; __graft_entry__.build() makes them
where the fitted code's tree is present).  For every case it

  1. runs ref_driver_san (ASan + UBSan, a stand-alone CPU program), which must exit clean: the proof that the fitted
     code is DEFINED on the case,
  2. runs ref_driver and requires the same bytes,
  3. checks the conditions on the generator's undefined-behaviour filter (share of replaced rows, rows left of the
     kind the case was built for),

and writes the results with every float and double as its bit pattern.  To keep the file small a case's inputs are
named by a sha256 digest rather than repeated: tests/reference_cases.py regenerates them and load() requires the digest.
Only data goes into the file: numbers the programs wrote while they ran.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import reference_cases as R  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
DRIVER = os.path.join(REF_DIR, "ref_driver")
DRIVER_SAN = os.path.join(REF_DIR, "ref_driver_san")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_parity.json")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def run_driver(driver, mode, blobs, tmp, tag):
    """One case through one build of the driver: the result file's bytes."""
    cpath, rpath = os.path.join(tmp, tag + ".case"), os.path.join(tmp, tag + ".result")
    R.write_blobs(cpath, blobs)
    p = subprocess.run([driver, mode, cpath, rpath], env=dict(os.environ, **SAN_ENV), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    if p.returncode != 0 or p.stdout:
        raise RuntimeError("%s %s: exit %d\n%s" % (os.path.basename(driver), tag, p.returncode, p.stdout.decode()))
    with open(rpath, "rb") as f:
        raw = f.read()
    return raw, R.read_blobs(rpath)


def check_filter(case):
    """The conditions on what the undefined-behaviour filter did to a pdfz case."""
    n, m = len(case["samples"]), len(case["points"])
    assert n <= R.MAX_SAMPLES and m <= R.MAX_POINTS, case["name"]
    assert len(case["replaced"]) <= R.MAX_REPLACED_SHARE * n, (case["name"], len(case["replaced"]), n)
    assert len(case["points_replaced"]) <= R.MAX_REPLACED_SHARE * m, (case["name"], len(case["points_replaced"]), m)
    assert len(case["built"]) >= R.MIN_BUILT_ROWS, (case["name"], len(case["built"]))


def record(drivers=(DRIVER_SAN, DRIVER)):
    """The fixture as a dict, every case run through every driver in `drivers` with identical bytes."""
    out = {"format": 1, "pdfz": [], "nll": []}
    with tempfile.TemporaryDirectory() as tmp:
        for family, cases, blobs_of, to_json in (("pdfz", R.pdfz_cases(), R.pdfz_blobs, R.pdfz_to_json),
                                                 ("nll", R.nll_cases(), R.nll_blobs, R.nll_to_json)):
            for case in cases:
                if family == "pdfz":
                    check_filter(case)
                runs = [run_driver(d, family, blobs_of(case), tmp, os.path.basename(d)) for d in drivers]
                for raw, _ in runs[1:]:
                    assert raw == runs[0][0], "the builds of the driver disagree on " + case["name"]
                out[family].append(to_json(case, runs[0][1]))
    return out


def dumps(fixture):
    """One case per line, keys sorted: a stable text for a byte-for-byte comparison."""
    lines = ['{"format": %d,' % fixture["format"]]
    for family in ("pdfz", "nll"):
        lines.append('"%s": [' % family)
        lines.append(",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in fixture[family]))
        lines.append("]," if family == "pdfz" else "]}")
    return "\n".join(lines) + "\n"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    for d in (DRIVER, DRIVER_SAN):
        if not os.path.exists(d):
            sys.exit("missing %s: build it with oracle/ref/Makefile (REF=<the fitted code's tree>)" % d)
    text = dumps(record())
    with open(out_path, "w") as f:
        f.write(text)
    fx = json.loads(text)
    print("%s: %d pdfz cases, %d nll cases, %d bytes; every case clean under ASan + UBSan" %
          (out_path, len(fx["pdfz"]), len(fx["nll"]), len(text)))


if __name__ == "__main__":
    main()
