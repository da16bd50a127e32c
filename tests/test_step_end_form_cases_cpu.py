"""CPU: the cases of tests/test_gpu_step_end_forms.py (tests/step_end_form_cases.py) are what the GPU tests take them for
-- asserted on the reference alone, with the oracle's set_eval_points and bin_samples: the exact number of event classes
of every case, its rows x members, its histogram words, and in every workload of three or more members a last member
with no sample inside.  Every case then sits on the intended side of the limits the step end's forms are chosen by:
blocks of 128 rows, 256 look-ups and 65 536 words for the one-workgroup form, 128 workers for the cooperative forms,
256 parameters for the staged finisher and the look-ahead pass.
"""
import numpy as np
import pytest

from tests import step_end_form_cases as cases


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=repr)
def test_case_is_what_it_says(case):
    w = case.workload()
    assert w.nsignals == case.members
    assert w.events.shape[0] == case.nevents
    assert cases.event_classes(w) == case.classes
    assert list(w.nbins) == list(case.nbins)
    assert case.words == sum(int(np.prod(w.nbins)) for _ in w.signals)
    assert case.lookups == (w.events.shape[0] if case.lut_output else case.classes) * w.nsignals
    norms = cases.nominal_norms(w)
    if case.members >= 3:
        assert norms[-1] == 0 and all(n > 0 for n in norms[:-1]), norms
    else:
        assert all(n > 0 for n in norms), norms
    if case.kind == "table":
        assert w.nparameters == w.nsources + 1 == max(case.members, 2)
        assert case.members < 3 or w.signals[1].source_id == w.signals[2].source_id      # two signals on one source
    else:
        assert w.nsources == case.members and w.nparameters == case.members + (case.kind == "parameters")
    # events outside every member and, in the table workloads of more than one class, of a data set no signal belongs to
    if case.kind == "table" and case.classes > 1:
        assert np.count_nonzero(w.events[:, -1] == 1.0) == 7 and np.count_nonzero(w.events[:, 0] == 99.0) == 8


def test_lookahead_cases_sit_on_both_sides_of_a_block_and_of_sixteen_members():
    got = [(c.members, c.classes, c.blocks) for c in cases.LOOKAHEAD]
    assert got == [(1, 300, 3), (12, 127, 1), (12, 128, 1), (12, 129, 2), (16, 300, 3), (17, 300, 3), (17, 129, 2)]
    for c in cases.LOOKAHEAD + [cases.FIXED] + cases.FUSED:
        # none of them ends in the one-workgroup form (the look-ahead pass would be refused), all of them cooperatively
        assert c.lookups > cases.TAIL_LOOKUPS and not c.one_workgroup and 2 * c.blocks <= cases.COOP_WORKERS
    assert [(c.members, c.classes) for c in cases.FUSED] == [(16, 300), (17, 300)]


def test_worker_limit_cases():
    at, beyond = cases.WORKERS_AT_LIMIT, cases.WORKERS_BEYOND
    assert (at.classes, at.blocks, 2 * at.blocks) == (8192, 64, cases.COOP_WORKERS)
    assert (beyond.classes, beyond.blocks) == (8193, 65) and 2 * beyond.blocks > cases.COOP_WORKERS
    assert beyond.blocks <= cases.COOP_WORKERS            # (the sequential step of that chain still ends cooperatively)
    for c in (at, beyond):
        assert c.members == 1 and c.words == 96 * 96 and not c.one_workgroup
        assert 2 * c.words * 4 < 128 * 1024               # two such histograms: inside a CU's 160 KiB of LDS


def test_parameter_limit_cases():
    a, b = cases.PARAMETERS_256.workload(), cases.PARAMETERS_257.workload()
    assert (a.nparameters, a.nsources, a.nsignals) == (256, 255, 255) and a.nparameters == cases.STAGED
    assert (b.nparameters, b.nsources, b.nsignals) == (257, 256, 256)
    assert len(a.systematics) == 1 and not cases.PARAMETERS_256.one_workgroup
    w = cases.FIXED.workload()
    assert w.nparameters == w.nsources + 1 == 12          # parameter 0: a rate; the last one: the systematic's


def test_one_workgroup_cases_sit_on_both_sides_of_its_limits():
    assert [(c.members, c.rows, c.lookups) for c in cases.TAIL_TAKEN] == [(16, 16, 256), (17, 15, 255), (1, 256, 256),
                                                                         (256, 1, 256)]
    assert [(c.members, c.rows, c.lookups) for c in cases.TAIL_NOT_TAKEN] == [(16, 17, 272), (1, 257, 257), (257, 1, 257)]
    for c in cases.TAIL_TAKEN:
        assert c.one_workgroup and c.words <= cases.TAIL_WORDS, c
    for c in cases.TAIL_NOT_TAKEN:
        # the look-ups alone keep them out: their histograms would fit
        assert not c.one_workgroup and c.words <= cases.TAIL_WORDS, c
    # 256 rows: two blocks of the sequential event sum, one workgroup here
    assert cases.TAIL_TAKEN[2].blocks == 2 and all(c.blocks == 1 for c in cases.TAIL_TAKEN[:2] + cases.TAIL_TAKEN[3:])
    # staged at exactly kStage: 256 members and 256 parameters; 257 of each are not staged
    w256, w257 = cases.TAIL_TAKEN[3].workload(), cases.TAIL_NOT_TAKEN[2].workload()
    assert (w256.nsignals, w256.nparameters) == (cases.STAGED, cases.STAGED)
    assert (w257.nsignals, w257.nparameters) == (cases.STAGED + 1, cases.STAGED + 1)
    yes, no = cases.TAIL_WORDS_TAKEN, cases.TAIL_WORDS_NOT_TAKEN
    assert yes.words == cases.TAIL_WORDS and yes.one_workgroup and yes.dense
    assert no.words == cases.TAIL_WORDS + 256 and not no.one_workgroup and no.dense
    assert yes.lookups == no.lookups == 100               # the words alone tell them apart
    lut = cases.TAIL_LUT
    assert lut.lut_output and (lut.rows, lut.classes, lut.lookups) == (16, 3, 256) and lut.one_workgroup


@pytest.mark.parametrize("members", cases.LOCKSTEP_MEMBERS)
def test_lockstep_chains_have_very_different_sizes(members):
    w = cases.lockstep_workload(members)
    assert w.nsignals == members and cases.nominal_norms(w)[-1] == 0
    blocks = []
    for chain, classes in enumerate(cases.LOCKSTEP_CLASSES):
        ev = cases.lockstep_events(members, classes, chain)
        assert cases.event_classes(w, ev) == classes
        assert not cases.takes_one_workgroup(classes, members, members * 400)
        blocks.append(cases.sum_blocks(classes))
    assert blocks == [1, 3, 2, 1] and len(blocks) == cases.MAX_LOCKSTEP
    small = cases.lockstep_events(members, cases.LOCKSTEP_SMALL, 9)
    assert cases.event_classes(w, small) == cases.LOCKSTEP_SMALL
    assert cases.takes_one_workgroup(cases.LOCKSTEP_SMALL, members, members * 400)
    assert sorted(cases.LOCKSTEP_SETS) == [(n, joint) for n in (2, 3, 4) for joint in (False, True)]


def test_stops_of_the_odd_pieces():
    assert sum(cases.PIECES[0]) == sum(cases.PIECES[1]) == 32 and cases.PIECES[0][:3] == (17, 1, 2)
    # by hand: refused + B | accepted | refused + B | refused with no step left before the stop
    assert cases.stops_reached_by([False, False, True, False, True, False], (2, 1, 2, 1)) == ["B", "A", "B", "A"]
    assert cases.stops_reached_by([True, False, False], (3,)) == ["B"]
    assert cases.stops_reached_by([False, False, False], (3,)) == ["A"]      # A+B, then an A-step alone
    assert cases.stops_reached_by([True] * 5, (2, 3)) == ["A", "A"]
