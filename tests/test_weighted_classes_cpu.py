"""CPU: the classes' weight sums of a group with event weights -- sxplan::class_weights beside sxplan::event_classes
(sxmc_amd/csrc/sxmc_plan.h, what ensure_event_classes uploads) -- through a stand-alone program with its own main
(tests/cpp/weighted_classes_host.cpp), plain and built with -fsanitize=address,undefined, against
tests/weighted_events_reference.py: the classes, their order, their counts and their weight sums, bit for bit.

The cases: no events; one; all events in one class; every event its own class; two members with different tables; and
weights whose sum depends on the order of addition (2^53 and ones: 2^53 + 1 + 1 is 2^53 added in that order and
2^53 + 2 with the ones first), which pins the ascending event index -- event_classes' std::sort is not stable.
Then the reference's own controls, and the refusal's index."""
import os
import subprocess

import numpy as np
import pytest

from tests import weighted_events_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = float(2 ** 53)


def _cases():
    rng = np.random.default_rng(11)
    out = {}
    out["no events"] = (np.zeros((2, 0), np.int64), np.zeros(0))
    out["one event"] = (np.array([[5], [5]]), np.array([0.75]))
    out["one class"] = (np.full((3, 40), 7), rng.uniform(0, 3, 40))
    out["every event its own"] = (np.stack([rng.permutation(50)] * 2), rng.uniform(0, 3, 50))
    a = rng.integers(-2, 6, 300)
    b = rng.integers(0, 3, 300)
    w = rng.uniform(0, 3, 300)
    w[rng.uniform(size=300) < 0.2] = 0.0
    out["two tables"] = (np.stack([a, b, a]), w)
    # the order of addition: in a class of many events (so that the sort moves them about) the big weight comes FIRST in
    # event order in class 3 and LAST in class 4
    t = np.concatenate([np.full(40, 3), np.full(40, 4)])
    w = np.ones(80)
    w[0] = BIG
    w[79] = BIG
    perm_free = np.stack([t, t])
    out["order of addition"] = (perm_free, w)
    # ... and the same classes interleaved, so that ascending INDEX is not the order inside the table
    idx = rng.permutation(80)
    inv_first, inv_last = int(np.min(np.nonzero(t[idx] == 3)[0])), int(np.max(np.nonzero(t[idx] == 4)[0]))
    w2 = np.ones(80)
    w2[inv_first] = BIG
    w2[inv_last] = BIG
    out["order of addition, interleaved"] = (np.stack([t[idx], t[idx]]), w2)
    out["all ones"] = (np.stack([a, b]), np.ones(300))
    out["integers"] = (np.stack([a, b]), rng.choice([1.0, 2.0, 3.0, 7.0], 300))
    return out


CASES = _cases()


def run_program(program, tables, w, tmp_path, name="case"):
    exe = os.path.join(ROOT, "tests", "cpp", program)
    assert os.path.exists(exe), "__graft_entry__.build() builds tests/cpp/%s (weighted.mk)" % program
    S, E = tables.shape
    lines = ["%d %d" % (S, E)] + [" ".join(str(int(x)) for x in row) for row in tables]
    lines.append(" ".join("%016x" % int(b) for b in np.asarray(w, np.float64).view(np.uint64)))
    src = tmp_path / (name.replace(" ", "_").replace(",", "") + ".in")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (name, p.returncode, p.stderr[-2000:])
    rows = p.stdout.strip().split("\n")
    K = int(rows[0])
    keys, counts, W = [], [], []
    for line in rows[1:1 + K]:
        f = line.split()
        keys.append([int(x) for x in f[:S]])
        counts.append(int(f[S]))
        W.append(int(f[S + 1], 16))
    assert rows[1 + K].startswith("bad ")
    return np.array(keys, np.int64).reshape(K, S), np.array(counts, np.uint32), np.array(W, np.uint64), int(rows[1 + K][4:])


@pytest.mark.parametrize("program", ["weighted_classes_host", "weighted_classes_host_asan"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_class_weights_equal_the_reference_bit_for_bit(program, name, tmp_path):
    tables, w = CASES[name]
    keys, counts, W, bad = run_program(program, tables, w, tmp_path, name)
    want_keys, _ = ref.classes(tables)
    assert np.array_equal(keys, want_keys), name
    assert np.array_equal(counts, ref.class_counts(tables)), name
    assert np.array_equal(W, ref.class_weights(tables, w).view(np.uint64)), name
    assert bad == -1


def test_the_cases_are_what_they_are_taken_for():
    assert ref.classes(CASES["no events"][0])[0].shape[0] == 0
    assert ref.classes(CASES["one class"][0])[0].shape[0] == 1
    assert ref.classes(CASES["every event its own"][0])[0].shape[0] == 50
    t, w = CASES["two tables"]
    assert ref.classes(t)[0].shape[0] > ref.classes(t[:1])[0].shape[0] > 1      # the second table splits classes
    W = ref.class_weights(t, w)
    zero_in_class = [k for k in range(W.size) if W[k] > 0 and np.any(w[ref.classes(t)[1] == k] == 0)]
    assert zero_in_class                                                       # zeros that share a class with a positive
    for name in ("order of addition", "order of addition, interleaved"):
        t, w = CASES[name]
        W = ref.class_weights(t, w)
        # big first: the ones are lost, one by one; big last: 39 + 2^53, a tie, rounds to the even 2^53 + 40
        assert W[0] == BIG and W[1] == BIG + 40.0, (name, W)
        # ... and the sum DOES depend on the order: descending index gives the other pair
        back = ref.class_weights(t[:, ::-1], w[::-1])
        assert back[0] == BIG + 40.0 and back[1] == BIG
    t, w = CASES["all ones"]
    assert np.array_equal(ref.class_weights(t, w), ref.class_counts(t).astype(np.float64))
    t, m = CASES["integers"]
    events = np.arange(t.shape[1])
    rep = ref.repeat_events(events, m)
    assert np.array_equal(ref.classes(t[:, rep])[0], ref.classes(t)[0])
    assert np.array_equal(ref.class_counts(t[:, rep]).astype(np.float64), ref.class_weights(t, m))


@pytest.mark.parametrize("program", ["weighted_classes_host", "weighted_classes_host_asan"])
@pytest.mark.parametrize("value,at", [(float("nan"), 3), (float("inf"), 0), (-1.0, 9), (-5e-324, 4)])
def test_the_first_weight_that_is_refused_is_named(program, value, at, tmp_path):
    w = np.ones(10)
    w[at] = value
    w[9] = -2.0 if at < 9 else value
    tables = np.zeros((1, 10), np.int64)
    _, _, _, bad = run_program(program, tables, w, tmp_path)
    assert bad == at == ref.check_weights(w)[0]


def test_weights_the_law_admits_are_not_refused(tmp_path):
    w = np.array([0.0, -0.0, 5e-324, 1.7976931348623157e308, 1.0])
    assert ref.check_weights(w) is None
    _, _, _, bad = run_program("weighted_classes_host", np.zeros((1, 5), np.int64), w, tmp_path)
    assert bad == -1


def test_a_weight_read_from_the_wrong_index_changes_the_sum():
    """The reference's own control: terms follow their rows."""
    s = np.array([2.0, 3.0, 5.0, 0.0])
    w = np.array([1.0, 0.5, 2.0, 4.0])
    right = sum(ref.event_terms(s, w))
    assert right == 1.0 * np.log(2.0) + 0.5 * np.log(3.0) + 2.0 * np.log(5.0)      # (s = 0: no term)
    assert sum(ref.event_terms(s, np.roll(w, 1))) != right
    with pytest.raises(ValueError):
        ref.event_terms(s, w[:3])
