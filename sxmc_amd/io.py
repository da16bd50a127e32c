"""Input / output formats either side of the hot path, ROOT-free.

  read_table              src/io/ttree_io.cpp:21-159   first TTree of a ROOT file -> row-major float matrix
                                                       + field names; here: an .npz with one 1-D array per
                                                       field (int / float / double / bool -> float32)
  read_dataset_to_samples src/signal.cpp:50-109        cuts + column packing [fields..., DATASET]
  load_config             src/config.cpp:19-297, observable.cpp, systematic.cpp, source.cpp
                                                       the reference's JSON schema (C-style comments allowed,
                                                       README.md:64-65)
  write_chain             src/sxmc.cpp:130-141, mcmc.cpp:100-114  the "ls" ntuple: one column per parameter
                                                       + "likelihood"; here an .npz with the same columns

Config parsing and file formats are not compute; they exist so that a fit described in the reference's
schema can be run end to end (run_config; `fit.samples` re-loads a saved chain instead of walking, as sxmc.cpp:84-94
does).  Plots and ROOT files are not supported.
"""
import ctypes as C
import json
import math
import os
import re

import numpy as np

from . import capi, workloads

TYPE_NAMES = ("shift", "scale", "ctscale", "resolution_scale")     # systematic.cpp:21-36


def strip_comments(text):
    """Remove // and /* */ comments outside strings."""
    out, i, n, in_str = [], 0, len(text), False
    while i < n:
        c = text[i]
        if in_str:
            out.append(c)
            if c == "\\" and i + 1 < n:
                out.append(text[i + 1])
                i += 1
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
            out.append(c)
        elif text.startswith("//", i):
            while i < n and text[i] != "\n":
                i += 1
            continue
        elif text.startswith("/*", i):
            i = text.index("*/", i) + 2
            continue
        else:
            out.append(c)
        i += 1
    return "".join(out)


def read_table(path):
    """-> (float32 matrix [n, nfields] row-major, field names).  One 1-D array per field in an .npz."""
    with np.load(path) as z:
        fields = list(z.files)
        cols = []
        for f in fields:
            a = np.asarray(z[f])
            if a.ndim != 1 or a.dtype.kind not in "iufb":
                raise ValueError("field %r of %s: only 1-D int/float/double/bool branches are supported" % (f, path))
            cols.append(a.astype(np.float32))
    n = cols[0].size if cols else 0
    if any(c.size != n for c in cols):
        raise ValueError("fields of %s differ in length" % path)
    return (np.stack(cols, axis=1) if cols else np.zeros((0, 0), np.float32)), fields


def write_table(path, matrix, fields):
    np.savez(path, **{f: np.asarray(matrix)[:, i] for i, f in enumerate(fields)})


def sample_multiplicities(weights, max_total=0):
    """Real sample weights as integer multiplicities on a power-of-two scale (sxmc_sample_multiplicities, the library's
    one implementation; host arithmetic only): (m uint32 [n], log2_scale, total).  Raises capi.SxmcError on a weight that
    is negative or not finite, or when nothing fits."""
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    m = np.zeros(w.size, np.uint32)
    k, total = C.c_int(0), C.c_ulonglong(0)
    capi.call("sxmc_sample_multiplicities", capi.ptr(w), w.size, int(max_total), capi.ptr(m), C.byref(k), C.byref(total))
    return m, k.value, total.value


def read_dataset_to_samples(dataset, dataset_fields, dataset_id, sample_fields, cuts, required=None, want_kept=False):
    """signal.cpp:50-109.  dataset: [n, len(dataset_fields)]; sample_fields ends with "DATASET";
    cuts: list of (field, lower, upper) -- an event is dropped when a cut field is < lower or > upper
    (bounds inclusive); when several cuts name one field the LAST one counts, as in the reference's lookup table
    (signal.cpp:57-69 overwrites the field's bounds cut by cut).
    required: how many of the leading sample fields must exist in the data set (default: all of them, the MC tables).
    A data set of real events carries no Monte Carlo truth branch: the reference maps such a field past the row
    (signal.cpp:72-77) and never looks at it again -- GetSamples keeps the observables only -- so for data sets
    (required = number of observables) a missing non-observable field is filled with 0 instead of being refused.
    Returns float32 [nkept, len(sample_fields)]."""
    dataset = np.asarray(dataset, np.float32)
    keep = np.ones(dataset.shape[0], bool)
    last = {}
    for field, lower, upper in cuts:
        last[field] = (lower, upper)
    for j, name in enumerate(dataset_fields):
        if name in last:
            lower, upper = last[name]
            col = dataset[:, j]
            keep &= ~((col < np.float64(lower)) | (col > np.float64(upper)))
    required = len(sample_fields) - 1 if required is None else required
    out = np.zeros((int(keep.sum()), len(sample_fields)), np.float32)
    kept = dataset[keep]
    for k, f in enumerate(sample_fields[:-1]):
        if f in dataset_fields:
            out[:, k] = kept[:, dataset_fields.index(f)]
        elif k < required:
            raise KeyError("sample field %r not in data set fields %r" % (f, dataset_fields))
    out[:, -1] = dataset_id
    if want_kept:    # ... and which rows passed the cuts (what a per-row column beside the table is cut with)
        return out, np.flatnonzero(keep)
    return out


class FitConfig:
    """What FitConfig::FitConfig (config.cpp:19-297) extracts, as plain Python data."""


def _number(v, what):
    """json::Value::asDouble of config.h: a JSON number or boolean, else "<what>: not a number"."""
    if not isinstance(v, (int, float)):
        raise ValueError("%s: not a number" % what)
    return float(v)


def signal_pdf(name, c, nobservables):
    """A signal's "pdf" ("hist", the default, or "kernel": pdfz.EvalKernel) and, for "kernel" only, "bandwidth_scale":
    one number for every fit observable or one per fit observable in fit-observable order, each positive and finite;
    absent: 1.0 each.  -> (pdf, bandwidth_scale list; empty for a histogram signal).  Same rules and messages as
    sxmc::detail::signal_pdf_from_json (config.h)."""
    who = "signal '%s': " % name
    pdf = c.get("pdf", "hist")
    if not isinstance(pdf, str):
        raise ValueError("pdf: not a string")
    if pdf not in ("hist", "kernel"):
        raise ValueError(who + 'unknown "pdf" "%s" ("hist" or "kernel")' % pdf)
    if "bandwidth_scale" not in c:
        return pdf, ([1.0] * nobservables if pdf == "kernel" else [])
    if pdf != "kernel":
        raise ValueError(who + '"bandwidth_scale" is only for "pdf": "kernel"')
    b = c["bandwidth_scale"]
    if isinstance(b, str) and b == "cv":       # chosen by cross-validation when the evaluator is built (signal_cv)
        return pdf, [1.0] * nobservables
    if isinstance(b, list):
        if len(b) != nobservables:
            raise ValueError(who + '"bandwidth_scale" has %d values for %d fit observables' % (len(b), nobservables))
        scale = [_number(v, "bandwidth_scale") for v in b]
    else:
        scale = [_number(b, "bandwidth_scale")] * nobservables
    if not all(math.isfinite(v) and v > 0 for v in scale):
        raise ValueError(who + '"bandwidth_scale" must be positive and finite')
    return pdf, scale


def signal_sensitivity(name, c, pdf):
    """A kernel signal's "bandwidth_sensitivity": the alpha of pdfz.EvalKernel's adaptive bandwidths, a number in
    [0, 1]; absent: 0.0, the fixed bandwidths.  Refused on a histogram signal.  Same rules and messages as
    sxmc::detail::signal_sensitivity_from_json (config.h)."""
    who = "signal '%s': " % name
    if "bandwidth_sensitivity" not in c:
        return 0.0
    if pdf != "kernel":
        raise ValueError(who + '"bandwidth_sensitivity" is only for "pdf": "kernel"')
    v = _number(c["bandwidth_sensitivity"], "bandwidth_sensitivity")
    if not (math.isfinite(v) and 0 <= v <= 1):
        raise ValueError(who + '"bandwidth_sensitivity" must be a number in [0, 1]')
    return v


def signal_cutoff(name, c, pdf):
    """A kernel signal's "bandwidth_cutoff": the cutoff radius R of pdfz.EvalKernel's pair sum in bandwidths
    (EvalKernel.SetCutoff): 0, or a number >= 1, infinity included; absent: 0.0, no cutoff.  Refused on a histogram
    signal.  Same rules and messages as sxmc::detail::signal_cutoff_from_json (config.h)."""
    who = "signal '%s': " % name
    if "bandwidth_cutoff" not in c:
        return 0.0
    if pdf != "kernel":
        raise ValueError(who + '"bandwidth_cutoff" is only for "pdf": "kernel"')
    v = _number(c["bandwidth_cutoff"], "bandwidth_cutoff")
    if not (v == 0.0 or v >= 1.0):
        raise ValueError(who + '"bandwidth_cutoff" must be 0 or a number >= 1')
    return v


def _integer(v, what):
    """json::Value::asInt of config.h."""
    d = _number(v, what)
    if not (math.isfinite(d) and d == math.floor(d) and abs(d) < 9.0e18):
        raise ValueError("%s: not an integer" % what)
    return int(d)


CV_KEYS = ("lo", "hi", "steps", "per_observable", "max_rows")


def signal_cv(name, c, pdf):
    """A kernel signal's cross-validated bandwidth scales: None unless "bandwidth_scale" is "cv", else the grid and
    the search as a dict(lo, hi, steps, per_observable, max_rows) -- the defaults of pdfz.CvOptions overridden by the
    optional object "bandwidth_cv".  "bandwidth_cv" is refused on a histogram signal, without "bandwidth_scale": "cv",
    with another key or with a bad grid.  Same rules and messages as sxmc::detail::signal_cv_from_json (config.h)."""
    who = "signal '%s': " % name
    is_cv = pdf == "kernel" and isinstance(c.get("bandwidth_scale"), str) and c["bandwidth_scale"] == "cv"
    cv = dict(lo=0.125, hi=4.0, steps=21, per_observable=True, max_rows=65536)
    if "bandwidth_cv" not in c:
        return cv if is_cv else None
    if pdf != "kernel":
        raise ValueError(who + '"bandwidth_cv" is only for "pdf": "kernel"')
    if not is_cv:
        raise ValueError(who + '"bandwidth_cv" needs "bandwidth_scale": "cv"')
    o = c["bandwidth_cv"]
    if not isinstance(o, dict):
        raise ValueError(who + '"bandwidth_cv" must be an object')
    for k in sorted(o, key=lambda k: k.encode()):
        if k not in CV_KEYS:
            raise ValueError(who + '"bandwidth_cv" has no key "%s"' % k)
    if "lo" in o:
        cv["lo"] = _number(o["lo"], "lo")
    if "hi" in o:
        cv["hi"] = _number(o["hi"], "hi")
    if "steps" in o:
        cv["steps"] = _integer(o["steps"], "steps")
    if "per_observable" in o:
        if not isinstance(o["per_observable"], (bool, int, float)):
            raise ValueError("per_observable: not a boolean")
        cv["per_observable"] = bool(o["per_observable"])
    if "max_rows" in o:
        cv["max_rows"] = _integer(o["max_rows"], "max_rows")
    if not 1 <= cv["steps"] <= 32:
        raise ValueError(who + "Cross-validation steps must be between 1 and 32.")
    if not (math.isfinite(cv["lo"]) and math.isfinite(cv["hi"]) and 0 < cv["lo"] <= cv["hi"]):
        raise ValueError(who + "Cross-validation grid needs 0 < lo <= hi, both finite.")
    if cv["max_rows"] < 0:
        raise ValueError(who + '"bandwidth_cv": "max_rows" must not be negative')
    return cv


def fit_proposal(fit):
    """The fit's "proposal" ("diagonal", the default, or "covariance": the correlated proposal of the walkers) and, for
    "covariance" only, "proposal_shrinkage": a number in (0, 1]; absent: 0.05.  -> (proposal, shrinkage).  A
    configuration without the keys loads as before.  Same rules and messages as sxmc::detail::fit_proposal_from_json
    (config.h)."""
    proposal = fit.get("proposal", "diagonal")
    if not isinstance(proposal, str):
        raise ValueError("proposal: not a string")
    if proposal not in ("diagonal", "covariance"):
        raise ValueError('fit: unknown "proposal" "%s" ("diagonal" or "covariance")' % proposal)
    if "proposal_shrinkage" not in fit:
        return proposal, 0.05
    if proposal != "covariance":
        raise ValueError('fit: "proposal_shrinkage" is only for "proposal": "covariance"')
    v = _number(fit["proposal_shrinkage"], "proposal_shrinkage")
    if not 0 < v <= 1:
        raise ValueError('fit: "proposal_shrinkage" must be a number in (0, 1]')
    return proposal, v


def fit_constraint_correlations(fit, names, sigmas):
    """The fit's "constraint_correlations": a list of groups {"parameters": [names], "matrix": [[...]]} that tie the
    Gaussian constraints of the named parameters together.  names, sigmas: the walk's parameter names (sources, then
    <systematic>_<j>) and constraint widths.  Groups are disjoint; each matrix is square, of its group's size.  The groups
    are scattered into the P x P identity and the whole is validated by sxmc_constraint_whitening (symmetric, unit
    diagonal, entries in [-1, 1], positive definite, no correlated parameter without a sigma).  -> rho [P, P] float64,
    or None without the key: such a configuration loads as before.  Same rules and messages as
    sxmc::detail::fit_constraint_correlations_from_json (config.h)."""
    if "constraint_correlations" not in fit:
        return None
    groups = fit["constraint_correlations"]
    if not isinstance(groups, list):
        raise ValueError('fit: "constraint_correlations" is not a list of groups')
    names = list(names)
    P = len(names)
    rho = np.eye(P)
    taken = [False] * P
    for g, grp in enumerate(groups):
        where = "fit: constraint_correlations[%d]: " % g
        if (not isinstance(grp, dict) or not isinstance(grp.get("parameters"), list)
                or not isinstance(grp.get("matrix"), list)):
            raise ValueError(where + 'a group is {"parameters": [names], "matrix": [[...]]}')
        index = []
        for name in grp["parameters"]:
            if not isinstance(name, str):
                raise ValueError("parameters[]: not a string")
            if name not in names:
                raise ValueError(where + 'unknown parameter "%s"' % name)
            at = names.index(name)
            if taken[at]:
                raise ValueError(where + 'parameter "%s" is already in a group' % name)
            taken[at] = True
            index.append(at)
        n = len(index)
        matrix = grp["matrix"]
        if len(matrix) != n or any(not isinstance(row, list) or len(row) != n for row in matrix):
            raise ValueError(where + '"matrix" must be %d x %d for its %d parameters' % (n, n, n))
        for r in range(n):
            for c in range(n):
                rho[index[r], index[c]] = _number(matrix[r][c], "matrix[][]")
    if P == 0:
        raise ValueError("fit: constraint_correlations: no parameters")
    from . import capi, nll
    try:
        nll.constraint_whitening(rho, np.asarray(sigmas, np.float64))
    except capi.SxmcError as e:
        raise ValueError("fit: constraint_correlations: " + e.msg) from None
    return rho


def parameter_names_and_sigmas(fc):
    """The walk's parameter vector as the loaders know it: sources, then <systematic>_<j> (mcmc.cpp:53-98)."""
    names = [s["name"] for s in fc.sources]
    sigmas = [float(s["sigma"]) for s in fc.sources]
    for s in fc.systematics:
        for j in range(s["npars"]):
            names.append("%s_%d" % (s["name"], j))
            sigmas.append(float(s["sigmas"][j]))
    return names, sigmas


ASIMOV_WITH_DATA = 'fit: "asimov" fits the expected data set: it cannot be combined with configured data sets'


def fit_asimov(fit, has_data):
    """The fit's "asimov" (a boolean; absent: false): fit exactly one data set, the Asimov one
    (ensemble.make_asimov_dataset).  Refused together with configured data sets.  A configuration without the key loads
    as before.  Same rules and messages as sxmc::detail::fit_asimov_from_json (config.h)."""
    v = fit.get("asimov", False)
    if isinstance(v, bool):
        asimov = v
    elif isinstance(v, (int, float)):
        asimov = v != 0
    else:
        raise ValueError("asimov: not a boolean")
    if asimov and has_data:
        raise ValueError(ASIMOV_WITH_DATA)
    return asimov


def load_config(path_or_text, base_dir=None):
    if os.path.exists(path_or_text):
        base_dir = base_dir or os.path.dirname(os.path.abspath(path_or_text))
        text = open(path_or_text).read()
    else:
        text = path_or_text
    root = json.loads(strip_comments(text))
    fit, pdfs = root["fit"], root["pdfs"]
    obs_params, sys_params = pdfs["observables"], pdfs.get("systematics", {})
    sig_params, src_params = root["signals"], root.get("sources", {})

    fc = FitConfig()
    fc.nexperiments = int(fit["nexperiments"])                    # config.cpp:43-49
    fc.nsteps = int(fit["nsteps"])
    assert fc.nexperiments > 0 and fc.nsteps > 0
    fc.error_type = fit.get("error_type", "contour")
    assert fc.error_type in ("contour", "projection")
    fc.burnin_fraction = float(np.float32(fit.get("burnin_fraction", 0.1)))     # (floats in the reference: asFloat())
    fc.debug_mode = bool(fit.get("debug_mode", False))
    fc.output_prefix = fit.get("output_prefix", "lspace")
    fc.seed = int(fit.get("seed", 0))
    fc.confidence = float(np.float32(fit.get("confidence", 0.683)))
    fc.signal_name = fit.get("signal_name", "")
    fc.samples = fit.get("samples", "")      # config.cpp:51: a saved chain to use INSTEAD of walking (sxmc.cpp:84-94)
    fc.proposal, fc.proposal_shrinkage = fit_proposal(fit)

    def observable(name):
        c = obs_params[name]
        return dict(name=name, field=c["field"], bins=int(c["bins"]), lower=np.float32(c["min"]),
                    upper=np.float32(c["max"]))

    fc.observables = [observable(n) for n in fit["observables"]]
    fc.cuts = [observable(n) for n in fit.get("cuts", [])]
    assert not {o["name"] for o in fc.observables} & {c["name"] for c in fc.cuts}

    # systematics and sources: union over the signals (config.cpp:97-151).  The reference walks the JSON object
    # `signals` with jsoncpp 0.6's iterator, i.e. in KEY order (a std::map compared with strcmp), not in file order:
    # the numbering of the sources and of the systematic parameters -- the layout of the parameter vector -- follows it
    fc.systematics, fc.sources = [], []
    pidx = 0
    for sname in sorted(sig_params, key=lambda k: k.encode()):
        sconf = sig_params[sname]
        for sys_name in sconf.get("systematics", []):
            if any(s["name"] == sys_name for s in fc.systematics):
                continue
            c = sys_params[sys_name]
            if c["type"] not in TYPE_NAMES:
                raise ValueError("Unknown systematic type %s" % c["type"])
            means = [float(x) for x in c["mean"]]
            sigmas = [float(x) for x in c["sigma"]] if "sigma" in c else [0.0] * len(means)
            assert len(sigmas) == len(means)
            s = dict(name=sys_name, type=c["type"], observable_field=c["observable_field"],
                     truth_field=c.get("truth_field") if c["type"] == "resolution_scale" else None,
                     means=means, sigmas=sigmas, npars=len(means), fixed=bool(c.get("fixed", False)),
                     pidx=list(range(pidx, pidx + len(means))))
            if c["type"] == "resolution_scale":
                assert s["truth_field"] is not None
            pidx += len(means)
            fc.systematics.append(s)
        if "source" in sconf:
            src_name = sconf["source"]
            if not any(s["name"] == src_name for s in fc.sources):
                p = src_params[src_name]
                fc.sources.append(dict(name=src_name, index=len(fc.sources), mean=np.float32(p.get("mean", 1.0)),
                                       sigma=np.float32(p.get("sigma", 0.0)), fixed=bool(p.get("fixed", False))))
        else:                                                   # the signal is a source for itself
            fc.sources.append(dict(name=sname, index=len(fc.sources), mean=np.float32(sconf.get("mean", 1.0)),
                                   sigma=np.float32(sconf.get("sigma", 0.0)), fixed=bool(sconf.get("fixed", False))))

    fc.constraint_correlation = fit_constraint_correlations(fit, *parameter_names_and_sigmas(fc))

    # order of the sampled fields: observables, then extra truth fields, then DATASET (config.cpp:153-194)
    fc.sample_fields = []

    def index_with_append(name):
        if name not in fc.sample_fields:
            fc.sample_fields.append(name)
        return fc.sample_fields.index(name)

    for o in fc.observables:
        o["field_index"] = index_with_append(o["field"])
    for s in fc.systematics:
        assert s["observable_field"] in fc.sample_fields, "systematic observable must be an observable"
        s["observable_field_index"] = fc.sample_fields.index(s["observable_field"])
        s["truth_field_index"] = index_with_append(s["truth_field"]) if s["type"] == "resolution_scale" else 0
    fc.sample_fields.append("DATASET")

    fc.signals = []
    for name in fit["signals"]:                                   # config.cpp:197-258
        c = sig_params[name]
        assert ("rate" in c) != ("scale" in c)
        src_name = c.get("source", name)
        pdf, bandwidth_scale = signal_pdf(name, c, len(fc.observables))
        # "weight_field": a field of the sample file holding one real weight per row (weighted Monte Carlo); not a
        # sample field: quantised over ALL rows of the file (sxmc_sample_multiplicities) and cut with the rows
        weight_field = c.get("weight_field", "")
        if not isinstance(weight_field, str):
            raise ValueError("weight_field: not a string")
        if weight_field:
            if pdf == "kernel":
                raise ValueError("signal '%s': \"weight_field\" is only for \"pdf\": \"hist\" (kernel-density weights "
                                 "are not built)" % name)
            if weight_field in fc.sample_fields:
                raise ValueError("signal '%s': weight_field '%s' is also an observable or a systematic's field"
                                 % (name, weight_field))
        fc.signals.append(dict(
            weight_field=weight_field,
            name=name, dataset=int(c["dataset"]), filename=c["filename"],
            # config.cpp:216-222: both go through a float
            rate=float(np.float32(c["rate"])) if "rate" in c else None,
            scale=float(np.float32(c["scale"])) if "scale" in c else None,
            systematics=[s for s in c.get("systematics", [])],
            source=next(s for s in fc.sources if s["name"] == src_name),
            pdf=pdf, bandwidth_scale=bandwidth_scale,
            bandwidth_sensitivity=signal_sensitivity(name, c, pdf),
            bandwidth_cv=signal_cv(name, c, pdf),
            bandwidth_cutoff=signal_cutoff(name, c, pdf)))
    fc.data = {int(k): [dict(filename=row["filename"], title=row.get("title", "")) for row in rows]
               for k, rows in root.get("data", {}).items()}
    fc.asimov = fit_asimov(fit, any(len(rows) > 0 for rows in fc.data.values()))
    fc.base_dir = base_dir or "."
    return fc


def build_workload(fc):
    """Load every signal's table (Signal::Signal, signal.cpp:11-47) and assemble the Workload the MCMC
    driver takes.  All signals must carry the same systematics list (one batched launch)."""
    nobs = len(fc.observables)
    nfields = len(fc.sample_fields)
    cuts = [(c["field"], c["lower"], c["upper"]) for c in fc.cuts]
    order = sorted(range(nobs), key=lambda i: fc.observables[i]["field_index"])
    signals = []
    for s in fc.signals:
        table, fields = read_table(os.path.join(fc.base_dir, s["filename"]))
        n_mc = table.shape[0]                                    # before cuts (signal.cpp:28)
        scale_by = float(n_mc)
        samples, kept = read_dataset_to_samples(table, fields, s["dataset"], fc.sample_fields, cuts, want_kept=True)
        multiplicities, log2_scale = None, 0
        if s.get("weight_field"):
            if s["weight_field"] not in fields:
                raise ValueError("signal '%s': weight_field '%s' is not a field of %s"
                                 % (s["name"], s["weight_field"], s["filename"]))
            weights = table[:, fields.index(s["weight_field"])].astype(np.float64)
            try:
                m, log2_scale, total = sample_multiplicities(weights)
            except capi.SxmcError as e:
                raise ValueError("signal '%s': weight_field '%s': %s" % (s["name"], s["weight_field"], e.msg))
            n_mc = total                                         # the multiplicities' total BEFORE cuts
            scale_by = float(np.ldexp(float(total), -log2_scale))    # "scale": the real weight total of the file
            multiplicities = m[kept]
        # config.cpp:221 keeps -1 / scale in a float, signal.cpp:31-35 multiplies it by -n_mc in double
        nexpected = s["rate"] if s["rate"] is not None else \
            float(np.float32(-1.0) / np.float32(s["scale"])) * (-1.0 * scale_by)
        # (bandwidth scales in the workload's observable order, that of lower / upper)
        scale = [s["bandwidth_scale"][i] for i in order] if s.get("bandwidth_scale") else None
        sig = workloads.Signal(samples, nfields, nexpected, s["source"]["index"], dataset=s["dataset"],
                               pdf=s.get("pdf", "hist"), bandwidth_scale=scale,
                               bandwidth_sensitivity=s.get("bandwidth_sensitivity", 0.0),
                               bandwidth_cv=s.get("bandwidth_cv"),
                               bandwidth_cutoff=s.get("bandwidth_cutoff", 0.0))
        sig.n_mc_total = n_mc
        sig.multiplicities, sig.weight_log2_scale = multiplicities, log2_scale
        sig.name = s["name"]
        signals.append(sig)
    systs = [dict(type=s["type"], obs=s["observable_field_index"], true_obs=s["truth_field_index"],
                  pars=s["pidx"]) for s in fc.systematics]
    lower = [float(fc.observables[i]["lower"]) for i in order]
    upper = [float(fc.observables[i]["upper"]) for i in order]
    nbins = [fc.observables[i]["bins"] for i in order]
    sigmas = [x for s in fc.systematics for x in s["sigmas"]]
    w = workloads.Workload(fc.output_prefix, nobs, lower, upper, nbins, signals, systs, sigmas,
                           np.zeros((0, nobs + 1), np.float32), "from config")
    w.source_means = [float(s["mean"]) for s in fc.sources]
    w.source_sigmas = [float(s["sigma"]) for s in fc.sources]
    w.syst_means = [x for s in fc.systematics for x in s["means"]]
    w.observable_names = [fc.observables[i]["name"] for i in order]
    w.parameter_names = [s["name"] for s in fc.sources] + \
        ["%s_%d" % (s["name"], j) for s in fc.systematics for j in range(s["npars"])] + ["likelihood"]
    nsrc = len(fc.sources)
    w.parameter_means = lambda: np.array(w.source_means + w.syst_means, np.float64)
    w.parameter_sigmas = lambda: np.array(w.source_sigmas + sigmas, np.float64)
    assert w.nsources == nsrc
    return w


def load_data(fc, w, experiment=0):
    """The data experiment i fits when the configuration lists data sets (config.cpp:261-296, sxmc.cpp:71-80): file i
    of EVERY data set, in the order of the data set ids, clipped to the PDF boundaries (observables act as cuts).
    None: no data sets configured (the caller samples a fake one)."""
    if not fc.data:
        return None
    cuts = [(o["field"], o["lower"], o["upper"]) for o in fc.observables] + \
           [(c["field"], c["lower"], c["upper"]) for c in fc.cuts]
    rows = []
    for dataset, files in sorted(fc.data.items()):
        if experiment >= len(files):        # (the reference indexes past the end of its list here)
            raise ValueError("data set %d lists %d file(s): experiment %d has none to fit (one file per experiment)"
                             % (dataset, len(files), experiment))
        f = files[experiment]
        table, fields = read_table(os.path.join(fc.base_dir, f["filename"]))
        s = read_dataset_to_samples(table, fields, dataset, fc.sample_fields, cuts, required=len(fc.observables))
        rows.append(np.concatenate([s[:, :w.nobs], s[:, -1:]], axis=1))      # GetSamples: observables + dataset
    return np.concatenate(rows, axis=0)


def write_chain(path, names, chain):
    """The "ls" ntuple of one experiment: columns = parameter names + "likelihood"."""
    np.savez(path, **{n: np.asarray(chain)[:, i] for i, n in enumerate(names)})


def _g17(v):
    return "%.17g" % float(v)


def write_fit_spectra(directory, spectra):
    """The result of ensemble.fit_spectra as one <observable name>_<dataset>.json per observable and data set in
    `directory` (created if missing) -- the file names of plot_fit (plots.cpp:297-299).  Each file is one object:
      observable, dataset, lower, upper, bins
      signals: [{name, nexp, spectrum: [bins numbers]}]   that data set's signals, in signal order
      fit: [bins numbers]      their sum
      data: [bins integers]    the data set's events, histogrammed
    Numbers are printed with 17 significant digits, so a double survives the round trip.  Returns the paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for sp in spectra:
        def arr(v):
            return "[" + ", ".join(_g17(x) for x in v) + "]"
        sigs = ",\n    ".join('{"name": %s, "nexp": %s, "spectrum": %s}'
                              % (json.dumps(str(g["name"])), _g17(g["nexp"]), arr(g["spectrum"])) for g in sp["signals"])
        text = ('{\n  "observable": %s,\n  "dataset": %d,\n  "lower": %s,\n  "upper": %s,\n  "bins": %d,\n'
                '  "signals": [\n    %s\n  ],\n  "fit": %s,\n  "data": [%s]\n}\n'
                % (json.dumps(str(sp["observable"])), int(sp["dataset"]), _g17(sp["lower"]), _g17(sp["upper"]),
                   int(sp["bins"]), sigs, arr(sp["fit"]), ", ".join(str(int(c)) for c in sp["data"])))
        path = os.path.join(directory, "%s_%d.json" % (sp["observable"], int(sp["dataset"])))
        with open(path, "w") as f:
            f.write(text)
        paths.append(path)
    return paths


def run_config(path, out_dir=None, nexperiments=None, nsteps=None, report=None, spectra_dir=None):
    """ensemble() of sxmc.cpp:44-145 for a config in the reference's schema: per experiment fake data
    (or the configured data sets), MCMC, contour intervals; chains written as <prefix>_<i>.npz.
    report: a text stream that receives, per experiment, what sxmc.cpp:100-101 prints (best fit + correlation matrix).
    spectra_dir: when given, experiment i's fit spectra at its point estimates (ensemble.fit_spectra: plot_fit,
    sxmc.cpp:104-107) are written to spectra_dir/<i>/ (write_fit_spectra); nothing is written otherwise, whatever the
    configuration's "plots" key says.
    Returns (intervals [nexp, P, 4], limits of fit.signal_name, parameter names)."""
    from . import ensemble

    def say(names, chain, iv, one_sided=None):
        if report is not None:
            report.write(ensemble.format_best_fit(names, iv, np.asarray(chain, np.float32)[:, -1].min(), fc.confidence, one_sided))
            report.write(ensemble.format_correlations(names, ensemble.correlation_matrix(chain)))
    fc = load_config(path)
    if fc.asimov and spectra_dir:
        raise ValueError('run_config: fit spectra of weighted events are not built: "asimov" cannot be combined with '
                         "spectra_dir")
    if fc.samples:                                               # sxmc.cpp:84-94: no walk, the saved likelihood space
        chain, names = read_table(os.path.join(fc.base_dir, fc.samples))
        assert names and names[-1] == "likelihood" and chain.shape[0] > 0
        one_sided = None
        if fc.error_type == "projection":
            cols = [ensemble.projection_interval(chain[:, p], fc.confidence) for p in range(len(names) - 1)]
            iv = np.array([c[:4] for c in cols], np.float32)
            one_sided = [bool(c[4]) for c in cols]
        else:
            iv = ensemble.contour_intervals(chain, fc.confidence)
        say(names[:-1], chain, iv, one_sided)
        limits = [float(iv[names.index(fc.signal_name), 2])] if fc.signal_name in names[:-1] else []
        return iv[None], limits, names
    from .mcmc import MCMC
    w = build_workload(fc)
    m = MCMC(w, seed=fc.seed & 0xFFFFFFFF, fused=True, lut_output=False, consume=True)
    nexp = 1 if fc.asimov else (nexperiments or fc.nexperiments)   # ("asimov": exactly one data set, the expected one)
    nsteps = nsteps or fc.nsteps
    allint, limits = [], []
    for i in range(nexp):
        rng = np.random.default_rng((fc.seed << 20) + i)
        events = load_data(fc, w, i)                             # sxmc.cpp:71-80: file i of every configured data set
        weights = None
        if fc.asimov:
            events, weights, _ = ensemble.make_asimov_dataset(w, m.pdfs)
            if report is not None:
                report.write("Fitting the Asimov data set: %d weighted rows, %.17g expected events\n"
                             % (events.shape[0], float(np.sum(weights))))
        elif events is None:
            events, _ = ensemble.make_fake_dataset(rng, w, m.pdfs, poisson=True)
        m.reseed(((fc.seed << 20) + i) & 0xFFFFFFFF)
        chain, _ = m.walk(events, nsteps, fc.burnin_fraction, debug_mode=fc.debug_mode, proposal=fc.proposal,
                          proposal_shrinkage=fc.proposal_shrinkage, event_weights=weights,
                          constraint_correlation=fc.constraint_correlation)
        if fc.error_type == "projection":                       # likelihood.cpp:104-137: the chosen estimator
            cols = [ensemble.projection_interval(chain[:, p], fc.confidence) for p in range(chain.shape[1] - 1)]
            iv = np.array([c[:4] for c in cols], np.float32)
        else:
            cols = None
            iv = ensemble.contour_intervals(chain, fc.confidence)
        say(w.parameter_names, chain, iv, [bool(c[4]) for c in cols] if cols else None)
        allint.append(iv)
        if fc.signal_name in w.parameter_names:
            limits.append(float(iv[w.parameter_names.index(fc.signal_name), 2]))
        if out_dir:
            write_chain(os.path.join(out_dir, "%s_%d.npz" % (fc.output_prefix, i)), w.parameter_names, chain)
        if spectra_dir:
            write_fit_spectra(os.path.join(spectra_dir, str(i)), ensemble.fit_spectra(w, m.pdfs, iv[:, 0], events))
    return np.array(allint), limits, w.parameter_names
