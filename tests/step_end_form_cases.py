"""The cases of tests/test_gpu_step_end_forms.py -- the look-ahead pass, the lockstep sets, the one-workgroup step end
and the fused step at the edges the sequential step end is tested at -- shared with tests/test_step_end_form_cases_cpu.py,
which asserts on the reference alone (the oracle's set_eval_points and bin_samples, no device) that every case is what
the GPU tests take it for: its event classes, its rows x members, its histogram words, its member of normalisation 0.
TEST INFRASTRUCTURE ONLY.  (tools/soak_lookahead.py and tools/soak_lockstep.py draw their workloads from here too.)

The workloads are those of tests/test_gpu_step_end_table.py (make_workload / make_events) and
tests/test_gpu_step_end_arith.py (workload(), the signals of many_sources()): about 3 000 samples per signal, events
in the low thousands -- the step end does not see the table size.  Only the worker limit needs more events than that: 8 192
classes are at least 8 192 events.

THE HOST'S RULES, restated here from their documentation (include/sxmc_hip.h, sxmc_group_step_async) so that the device-free
check can say which side of a limit a case is on:
  * the event sum is cut into blocks of 128 rows, at most 1 024 of them;
  * the one-workgroup step end takes problems of at most 256 look-ups (rows x members) over at most 65 536 histogram words;
  * the cooperative step ends have at most 128 workers: 128 blocks of one candidate, or 64 of each of the look-ahead's two;
  * the look-ahead pass and the finisher's staged form hold at most 256 parameters (and signals).
"""
import functools

import numpy as np

from oracle import oracle
from sxmc_amd import workloads
from tests.test_gpu_step_end_arith import many_sources, workload
from tests.test_gpu_step_end_table import HI, LO, make_events

BLOCK_ROWS, MAX_BLOCKS = 128, 1024
TAIL_LOOKUPS, TAIL_WORDS = 256, 1 << 16
COOP_WORKERS = 128
STAGED = 256
MAX_LOCKSTEP = 4                      # SXMC_MAX_LOCKSTEP


def sum_blocks(rows):
    return min(MAX_BLOCKS, max(1, (rows + BLOCK_ROWS - 1) // BLOCK_ROWS))


def takes_one_workgroup(rows, members, words):
    return rows * members <= TAIL_LOOKUPS and words <= TAIL_WORDS


class Case:
    """members x classes over nbins.  `rows`: what the step end walks -- the classes, or with lut_output the events."""

    def __init__(self, members, classes, nbins=(20, 20), nevents=1500, lut_output=False, dense=False, prebinning=True,
                 kind="table"):
        self.members, self.classes, self.nbins, self.nevents = members, classes, tuple(nbins), nevents
        self.lut_output, self.dense, self.prebinning, self.kind = lut_output, dense, prebinning, kind

    def __repr__(self):
        return "%s%dx%d@%dx%d%s" % ("" if self.kind == "table" else self.kind + ":", self.members, self.classes,
                                    self.nbins[0], self.nbins[1], "+lut" if self.lut_output else "")

    @property
    def rows(self):
        return self.nevents if self.lut_output else self.classes

    @property
    def words(self):
        return self.members * self.nbins[0] * self.nbins[1]

    @property
    def lookups(self):
        return self.rows * self.members

    @property
    def blocks(self):
        return sum_blocks(self.rows)

    @property
    def one_workgroup(self):
        return takes_one_workgroup(self.rows, self.members, self.words)

    def workload(self):
        return _workload(self.kind, self.members, self.classes, self.nbins, self.nevents)


@functools.lru_cache(maxsize=None)
def _workload(kind, members, classes, nbins, nevents):
    """Built once, shared, never modified.
    "table": tests/test_gpu_step_end_arith.py's workload() -- members - 1 sources (signals 1 and 2 share one) and a scale
    systematic, from three members on a last member of normalisation 0.
    Hundreds of members (make_workload's signals move up the first observable and leave the histogram from the thirtieth
    on): the signals of many_sources() of that file, all inside, every one its own source -- here with a last member
    whose samples are moved out of the histogram, and events of `classes` classes over `nbins`.  "sources": no
    systematic, as many parameters as members; "parameters": a scale systematic besides, members + 1 parameters."""
    if kind == "table":
        return workload(members, classes, nbins, nevents=nevents)
    signals = many_sources(members).signals
    last = signals[-1]
    outside = last.samples.copy()
    outside[:, 0] += 50.0
    signals[-1] = workloads.Signal(outside, last.nfields, nexpected=last.nexpected, source_id=last.source_id)
    systs, sigmas = ([dict(type="scale", obs=0, pars=[0])], [0.01]) if kind == "parameters" else ([], [])
    events = make_events(np.random.default_rng(23), nbins, classes, nevents)
    return workloads.Workload(kind, 2, LO, HI, list(nbins), signals, systs, sigmas, events,
                              "%d members, %d event classes" % (members, classes))


def event_classes(w, events=None):
    """The distinct tuples of event bins over the members, from the oracle's set_eval_points."""
    events = w.events if events is None else events
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    per_dataset = {}
    for s in w.signals:
        if s.dataset not in per_dataset:
            per_dataset[s.dataset] = np.asarray(oracle.set_eval_points(geom, events, s.dataset))
    tuples = np.stack([per_dataset[s.dataset] for s in w.signals], axis=1)
    return np.unique(tuples, axis=0).shape[0]


def nominal_norms(w):
    """Every member's normalisation at the parameters' means."""
    geom = oracle.HistGeometry(w.lower, w.upper, w.nbins)
    at = w.parameter_means()[w.nsources:]
    return [int(oracle.bin_samples(geom, s.samples, s.nfields, w.systematics, at)[1]) for s in w.signals]


# ---------------------------------------------------------------------------------------------- (a) the look-ahead pass
# members x classes on each side of the member loop's sixteen and of a block of 128 rows
LOOKAHEAD = [Case(1, 300), Case(12, 127), Case(12, 128), Case(12, 129), Case(16, 300), Case(17, 300), Case(17, 129)]
# 64 blocks per candidate: the finisher's 128 lanes all poll; 65: the two-launch end although the switch is on.  One
# member over 96 x 96 bins (two such histograms fit LDS).  The planner would stream this table's untouched observable as
# a pre-binned column, a form of the fill the pass is not offered for: pre-binning is switched off for these two
WORKERS_AT_LIMIT = Case(1, 8192, (96, 96), nevents=9000, prebinning=False)
WORKERS_BEYOND = Case(1, 8193, (96, 96), nevents=9000, prebinning=False)
# one walk's steps, flush by flush, cut into stops: some reached by an A-step, some by a B-step (stops_reached_by)
PIECES = [(17, 1, 2, 3, 2, 7), (1, 3, 5, 2, 4, 17)]
FIXED = Case(12, 300)                             # walked with parameter 0 and the systematic fixed
PARAMETERS_256 = Case(255, 300, kind="parameters")          # 255 rates and the systematic's: staged at exactly kStage
PARAMETERS_257 = Case(256, 300, kind="parameters")


def stops_reached_by(accepted, pieces):
    """Which step of a pass reached each stop: a pass decides its A-step and, if that was refused and the stop allows
    one more, the following B-step.  accepted: the chain's decisions, step by step; pieces: steps between the stops.
    Returns one "A" or "B" per piece."""
    out, pos = [], 0
    for piece in pieces:
        cap, last = pos + piece, "A"
        while pos < cap:
            if not accepted[pos] and pos + 1 < cap:
                pos, last = pos + 2, "B"
            else:
                pos, last = pos + 1, "A"
        out.append(last)
    return out

# ---------------------------------------------------------------------------------------------- (c) the one-workgroup end
# (members, classes): rows x members on each side of 256
TAIL_TAKEN = [Case(16, 16, nevents=400), Case(17, 15, nevents=420), Case(1, 256, nevents=700),
              Case(256, 1, (10, 10), nevents=200, kind="sources")]
TAIL_NOT_TAKEN = [Case(16, 17, nevents=400), Case(1, 257, nevents=700),
                  Case(257, 1, (10, 10), nevents=200, kind="sources")]
# histogram words on each side of 65 536: one member, dense histograms (a histogram beyond LDS is by default counted in its
# event bins only -- a few words)
TAIL_WORDS_TAKEN = Case(1, 100, (256, 256), nevents=700, dense=True)
TAIL_WORDS_NOT_TAKEN = Case(1, 100, (256, 257), nevents=700, dense=True)
# rows are the events themselves, every member stores its lookup-table row: 16 x 16 = 256 look-ups
TAIL_LUT = Case(16, 3, nevents=16, lut_output=True)

# ---------------------------------------------------------------------------------------------- (b) lockstep sets
# chains over shared tables, each with events of its own: 1, 3, 2 and 1 blocks in one set
LOCKSTEP_MEMBERS = [16, 17]
LOCKSTEP_CLASSES = [40, 300, 129, 128]
LOCKSTEP_SMALL = 12                               # classes of a chain whose step ends in the one-workgroup form
# (nchains, joint ends): every one walked eager and replayed
LOCKSTEP_SETS = [(n, joint) for n in (2, 3, 4) for joint in (True, False)]


def lockstep_workload(members):
    return _workload("table", members, 300, (20, 20), 1500)


@functools.lru_cache(maxsize=None)
def lockstep_events(members, classes, chain):
    """Chain `chain`'s own events in exactly `classes` classes (make_events: classes - 1 bins and the events outside)."""
    ev = make_events(np.random.default_rng(1000 * members + 10 * classes + chain), (20, 20), classes, 600 + 100 * chain)
    ev.setflags(write=False)
    return ev


# ---------------------------------------------------------------------------------------------- (d) the fused step
FUSED = [Case(16, 300), Case(17, 300)]

ALL_CASES = (LOOKAHEAD + [WORKERS_AT_LIMIT, WORKERS_BEYOND, FIXED, PARAMETERS_256, PARAMETERS_257] + TAIL_TAKEN +
             TAIL_NOT_TAKEN + [TAIL_WORDS_TAKEN, TAIL_WORDS_NOT_TAKEN, TAIL_LUT] + FUSED)


# ---------------------------------------------------------------------------------------------- the soak tools' workloads
SOAK_LOOKAHEAD = LOOKAHEAD + [FIXED, WORKERS_AT_LIMIT, WORKERS_BEYOND]


def soak_case(rng):
    """A random case of the look-ahead pass's for tools/soak_lookahead.py."""
    return SOAK_LOOKAHEAD[int(rng.integers(0, len(SOAK_LOOKAHEAD)))]


def soak_lockstep(rng, nchains):
    """(workload, [events per chain]) for tools/soak_lockstep.py: 16 or 17 members, chains of very different sizes."""
    members = LOCKSTEP_MEMBERS[int(rng.integers(0, len(LOCKSTEP_MEMBERS)))]
    classes = [LOCKSTEP_CLASSES[int(i)] for i in rng.permutation(len(LOCKSTEP_CLASSES))[:nchains]]
    return lockstep_workload(members), [lockstep_events(members, k, c) for c, k in enumerate(classes)]
