"""THE LAW OF WEIGHTED DATA EVENTS, written down once (include/sxmc_hip.h states it beside sxmc_group_set_event_weights).
TEST INFRASTRUCTURE ONLY: plain numpy and Python floats, no device, nothing of the library.

  * event i has a weight w_i, a finite double >= 0;
  * the log-likelihood's event term is sum_i w_i log(s_i), s_i exactly the unweighted s: per signal j in order,
    s += coef_j * (double)(lut[j][i], NaN read as 0), coef_j = pars[source_id[j]] * nexpected[j] * (float)(norms[j] / n_mc[j]);
    events with s_i <= 0 add nothing;
  * rows are CLASSES (events with the same bin in every member): the class weight is W_k = sum of w_i over the events
    of class k in ASCENDING EVENT INDEX, in double, added one by one; the row's term is W_k * log(s_k), rounded once;
  * rows are EVENTS: the term is w_i * log(s_i).
Two exact consequences: all weights 1.0 give W_k == (double)n_k; integer weights m_i give the multiplicities of the data
set in which event i is repeated m_i times (repeat_events), whose classes and their order are the same.

The order of the CLASSES is the library's: ascending tuples of event bins, members in order.  The order in which rows'
terms are added is the kernels' partition and is not restated here: sums are compared to a tolerance (the f64 sum below
is math.fsum, correctly rounded), bytes are compared between two runs of the library.
"""
import math

import numpy as np


def check_weights(w):
    """None, or (index, why) of the first weight that is not a finite double >= 0."""
    for i, x in enumerate(np.asarray(w, np.float64).reshape(-1)):
        if math.isnan(x) or math.isinf(x) or x < 0:
            return i, "not a finite number >= 0"
    return None


def classes(tables):
    """tables: [S][E] event bins per member.  Returns (keys [K][S] ascending, class_of [E])."""
    t = np.asarray(tables, np.int64)
    if t.ndim != 2:
        raise ValueError("tables must be [S][E]")
    S, E = t.shape
    if E == 0:
        return np.zeros((0, S), np.int64), np.zeros(0, np.int64)
    keys, class_of = np.unique(t.T, axis=0, return_inverse=True)    # (rows sorted lexicographically: member 0 first)
    return keys, np.asarray(class_of).reshape(-1)


def class_weights(tables, w):
    """W[k]: the law's sum -- ascending event index, one addition at a time, in double."""
    keys, class_of = classes(tables)
    w = np.asarray(w, np.float64).reshape(-1)
    if w.size != class_of.size:
        raise ValueError("%d weights for %d events" % (w.size, class_of.size))
    W = [0.0] * keys.shape[0]
    for i in range(w.size):                                          # (Python floats: IEEE doubles, no pairwise summation)
        W[class_of[i]] = W[class_of[i]] + float(w[i])
    return np.array(W, np.float64)


def class_counts(tables):
    keys, class_of = classes(tables)
    return np.bincount(class_of, minlength=keys.shape[0]).astype(np.uint32)


def repeat_events(events, m):
    """The data set in which event i stands m[i] times (m: integers >= 1), in place."""
    m = np.asarray(m)
    if np.any(m < 1) or np.any(m != np.floor(m)):
        raise ValueError("repeat_events: integers >= 1")
    return np.ascontiguousarray(np.repeat(np.asarray(events), m.astype(np.int64), axis=0))


def coefficients(pars, nexpected, n_mc, source_id, norms):
    out = []
    for j in range(len(nexpected)):
        eff = float(np.float32(1.0 * float(norms[j]) / float(n_mc[j])))
        out.append(float(pars[int(source_id[j])]) * float(nexpected[j]) * eff)
    return out


def event_s(lut, coef):
    """s_i for every event: lut [S][E] float32, terms added in signal order in double."""
    lut = np.asarray(lut, np.float32)
    S, E = lut.shape
    s = np.zeros(E, np.float64)
    for j in range(S):
        v = np.where(np.isnan(lut[j]), np.float32(0), lut[j]).astype(np.float64)
        s = s + coef[j] * v
    return s


def event_terms(s, w):
    """[w_i * log(s_i)] with the s > 0 guard; w indexed like s."""
    s = np.asarray(s, np.float64)
    w = np.asarray(w, np.float64)
    if s.shape != w.shape:
        raise ValueError("one weight per row")
    return [float(w[i]) * math.log(float(s[i])) if s[i] > 0 else 0.0 for i in range(s.size)]


def weighted_event_sum(lut, pars, nexpected, n_mc, source_id, norms, w):
    """sum_i w_i log(s_i), correctly rounded."""
    return math.fsum(event_terms(event_s(lut, coefficients(pars, nexpected, n_mc, source_id, norms)), w))


def chunk_sums(lut, pars, nexpected, n_mc, source_id, norms, w, grid, block):
    """The launch point's partial sums: lane t adds its events t, t + grid * block, ... in index order."""
    terms = event_terms(event_s(lut, coefficients(pars, nexpected, n_mc, source_id, norms)), w)
    lanes = grid * block
    out = np.zeros(lanes, np.float64)
    for t in range(min(lanes, len(terms))):
        acc = 0.0
        for i in range(t, len(terms), lanes):
            acc += terms[i]
        out[t] = acc
    return out

