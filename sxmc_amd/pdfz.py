"""Python spelling of the reference's pdfz interface (src/pdfz.h) over the C ABI.

Same class names, method names, argument order and error behaviour as pdfz::Eval /
pdfz::EvalHist (pdfz.h:246-574): constructor validation raises `Error` where the reference
throws pdfz::Error; buffers are device arrays (capi.DeviceArray, or anything with data_ptr());
EvalAsync returns before completion and EvalFinished waits.  ROOT-returning methods
(CreateHistogram, CreateHistogramProjection, RandomSample) are replaced by plain-array accessors (GetBins, Project).
"""
import ctypes as C

import numpy as np

from . import capi


class Error(Exception):
    """pdfz::Error (pdfz.h:93-102)."""

    def __init__(self, msg):
        super().__init__(msg)
        self.msg = msg


class Systematic:
    SHIFT, SCALE, RESOLUTION_SCALE, CTSCALE = 0, 1, 2, 3   # pdfz.h:111-116

    def __init__(self, type_):
        self.type = type_


def _pars(pars):
    return [int(pars)] if np.isscalar(pars) else [int(p) for p in pars]


class ShiftSystematic(Systematic):
    """x' = x + p, p = sum p_i x^i (pdfz.h:145-157).  pars: parameter indices."""

    def __init__(self, obs, pars):
        super().__init__(Systematic.SHIFT)
        self.obs, self.pars = int(obs), _pars(pars)


class ScaleSystematic(Systematic):
    """x' = x (1 + p) (pdfz.h:168-180)."""

    def __init__(self, obs, pars):
        super().__init__(Systematic.SCALE)
        self.obs, self.pars = int(obs), _pars(pars)


class CosThetaScaleSystematic(Systematic):
    """x' = 1 + (x - 1)(1 + p) (pdfz.h:194-206)."""

    def __init__(self, obs, pars):
        super().__init__(Systematic.CTSCALE)
        self.obs, self.pars = int(obs), _pars(pars)


class ResolutionScaleSystematic(Systematic):
    """x' = x + p (x - x_true) (pdfz.h:218-233)."""

    def __init__(self, obs, true_obs, pars):
        super().__init__(Systematic.RESOLUTION_SCALE)
        self.obs, self.true_obs, self.pars = int(obs), int(true_obs), _pars(pars)


def _raise(rc):
    if rc == capi.ERR_INVALID:
        raise Error(capi.last_error())
    capi.check(rc)


class _Eval:
    """pdfz::Eval (pdfz.h:246-395): what EvalHist and EvalKernel have in common, over the entry points named
    `_prefix` + name.  A subclass's constructor hands its sxmc_*_create to _create."""

    _prefix = None

    def _call(self, name, *args):
        _raise(getattr(capi.load(), self._prefix + name)(self._h, *args))

    def _get(self, name, ctype):
        v = ctype(0)
        self._call(name, C.byref(v))
        return v.value

    def _create(self, create, samples, nfields, nobservables, lower, upper, extra, dataset):
        """create(samples, nfloats, on_device, nfields, nobservables, lower, n, upper, n, extra, n, dataset, &handle):
        the shape of sxmc_hist_create (extra = nbins) and sxmc_kde_create (extra = bandwidth scales)."""
        self._h = None
        on_device = hasattr(samples, "data_ptr")
        if on_device:
            nfloats = int(samples.numel())
        else:
            samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
            nfloats = samples.size
        lower = np.ascontiguousarray(lower, dtype=np.float64)
        upper = np.ascontiguousarray(upper, dtype=np.float64)
        h = C.c_void_p(0)
        _raise(create(capi.ptr(samples), nfloats, int(on_device), int(nfields), int(nobservables),
                      capi.ptr(lower), lower.size, capi.ptr(upper), upper.size, capi.ptr(extra), extra.size,
                      int(dataset), C.byref(h)))
        self._h = h
        self.nfields, self.nobservables, self.dataset = int(nfields), int(nobservables), int(dataset)
        self._keep = {}

    @classmethod
    def Shared(cls, base):
        """A second evaluator over the SAME sample table as `base` (nothing copied but the systematics, and a
        kernel density's bandwidths; own histogram or rows, points, bindings and stream): for concurrent chains /
        experiments on one GPU (sxmc_hist_create_shared, sxmc_kde_create_shared).  An EvalKernel's may
        outlive a closed `base`; an EvalHist's keeps `base` alive."""
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p(0)
        _raise(getattr(capi.load(), cls._prefix + "create_shared")(base._h, C.byref(h)))
        self._h = h
        self.nfields, self.nobservables, self.dataset = base.nfields, base.nobservables, base.dataset
        self._keep = {}
        return self

    def SetEvalPoints(self, points):
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1)
        self._call("set_eval_points", capi.ptr(points), points.size)

    def SetPDFValueBuffer(self, output, offset=0, stride=1):
        self._keep["pdf"] = output
        self._call("set_pdf_value_buffer", capi.ptr(output), int(offset), int(stride))

    def SetNormalizationBuffer(self, norm, offset=0):
        self._keep["norm"] = norm
        self._call("set_normalization_buffer", capi.ptr(norm), int(offset))

    def SetParameterBuffer(self, params, offset=0, stride=1):
        self._keep["params"] = params
        self._call("set_parameter_buffer", capi.ptr(params), int(offset), int(stride))

    def AddSystematic(self, syst):
        pars = np.asarray(syst.pars, dtype=np.int16)
        extra = getattr(syst, "true_obs", 0)
        self._call("add_systematic", int(syst.type), int(syst.obs), int(extra), pars.size, capi.ptr(pars))

    def EvalAsync(self, do_eval_pdf=True):
        self._call("eval_async", int(bool(do_eval_pdf)))

    def EvalFinished(self):
        self._call("eval_finished")

    def Optimize(self):
        pass

    def Project(self, obs, nbins):
        """The share of the PDF of the last evaluation in each of `nbins` equal bins of observable `obs` (float64; sums
        to 1, or all 0 when the norm is 0) -- CreateHistogramProjection (pdfz.h:505-518) without ROOT, computed on the
        device."""
        raise Error("Project is not implemented by this evaluator")

    def RandomSample(self, nobserved, seed, lowers=None, uppers=None):
        """EvalHist::RandomSample's sampling step on the device (pdfz.cpp:817-922): nobserved events drawn from the
        PDF of the last evaluation -- a histogram's bins (EvalAsync(False) first) or a kernel density's moved samples
        (EvalAsync first) -- rows of nobservables + 1 floats (last = dataset id); redrawn while outside
        [lowers, uppers] when given."""
        out = np.empty((int(nobserved), self.nobservables + 1), dtype=np.float32)
        lo = None if lowers is None else np.ascontiguousarray(lowers, dtype=np.float32)
        hi = None if uppers is None else np.ascontiguousarray(uppers, dtype=np.float32)
        self._call("random_sample", int(nobserved), int(seed) & 0xFFFFFFFFFFFFFFFF, capi.ptr(lo), capi.ptr(hi),
                   capi.ptr(out))
        return out

    @property
    def nsamples(self):
        return self._get("nsamples", C.c_size_t)

    @property
    def npoints(self):
        return self._get("npoints", C.c_size_t)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            getattr(capi.load(), self._prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EvalHist(_Eval):
    """pdfz::EvalHist (pdfz.h:402-574, pdfz.cpp:179-495)."""

    _prefix = "sxmc_hist_"

    def __init__(self, samples, nfields, nobservables, lower, upper, nbins, dataset=0, optimize=True):
        nbins = np.ascontiguousarray(nbins, dtype=np.int32)
        self._create(capi.load().sxmc_hist_create, samples, nfields, nobservables, lower, upper, nbins, dataset)
        self._nbins = [int(b) for b in nbins]

    @classmethod
    def Shared(cls, base):
        self = super().Shared(base)
        self._keep["base"] = base
        self._nbins = list(base._nbins)
        return self

    def ProjectCounts(self, obs):
        """The bins of the last evaluation summed over every observable but `obs` (uint64, exact), on the device:
        only the marginal comes back (sxmc_hist_project)."""
        obs = int(obs)
        if not 0 <= obs < self.nobservables:
            raise Error("no such observable to project onto")
        out = np.zeros(self._nbins[obs], dtype=np.uint64)
        self._call("project", obs, capi.ptr(out), out.size)
        return out

    def Project(self, obs, nbins):
        """counts / sum of counts along `obs`; nbins must be the evaluator's own bin count there."""
        if not 0 <= int(obs) < self.nobservables or int(nbins) != self._nbins[int(obs)]:
            raise Error("EvalHist projects onto its own bins: observable %d has %s, not %d"
                        % (obs, self._nbins[int(obs)] if 0 <= int(obs) < self.nobservables else "no bins", nbins))
        counts = self.ProjectCounts(obs)
        total = int(counts.sum())
        return counts / float(total) if total else np.zeros(counts.size)

    # -- weighted Monte Carlo samples: integer multiplicities (include/sxmc_hip.h) -------------
    def SetSampleMultiplicities(self, m):
        """One uint32 per table row: the fill adds m_i where it added 1 (sxmc_hist_set_sample_multiplicities).  Before the
        first evaluation and before the evaluator joins a group; a total beyond 2^32 - 1 raises Error."""
        if hasattr(m, "data_ptr"):
            n, on_device = int(m.numel()), 1
        else:
            m = np.ascontiguousarray(m)
            if m.dtype != np.uint32:
                if m.size and (np.any(m < 0) or np.any(m > 0xFFFFFFFF) or np.any(m != np.floor(m))):
                    raise Error("sample multiplicities are integers in [0, 2^32 - 1]")
                m = m.astype(np.uint32)
            m = m.reshape(-1)
            n, on_device = m.size, 0
        self._call("set_sample_multiplicities", capi.ptr(m), n, on_device)

    def SampleTotal(self):
        """The multiplicities' total, or the row count when none are set: n_mc for either kind."""
        return self._get("sample_total", C.c_ulonglong)

    def SampleMultiplicities(self):
        """The multiplicities (uint32 [nsamples]); all 1 when none are set."""
        out = np.empty(self.nsamples, dtype=np.uint32)
        self._call("get_sample_multiplicities", capi.ptr(out), out.size, None)
        return out

    # -- replaces Optimize*: analytic launch sizing, optionally overridden -------------------
    def SetLaunchConfig(self, bin_threads=0, bin_blocks_per_cu=0):
        self._call("set_launch_config", int(bin_threads), int(bin_blocks_per_cu))

    # -- introspection ----------------------------------------------------------------------
    @property
    def total_nbins(self):
        return self._get("total_nbins", C.c_int)

    @property
    def bin_volume(self):
        return self._get("bin_volume", C.c_double)

    def GetBins(self):
        """Bin contents of the last evaluation (the array CreateHistogram reads, pdfz.cpp:511)."""
        out = np.empty(self.total_nbins, dtype=np.uint32)
        self._call("get_bins", capi.ptr(out), out.size)
        return out

    def GetReadBins(self):
        out = np.empty(self.npoints, dtype=np.int32)
        self._call("get_read_bins", capi.ptr(out), out.size)
        return out

    def GetSamples(self):
        """pdfz.h:542-556: rows of nobservables + 1 floats (observables, dataset id)."""
        out = np.empty(self.nsamples * (self.nobservables + 1), dtype=np.float32)
        self._call("get_samples", capi.ptr(out), out.size)
        return out


def _multiplicities(m):
    """One uint32 per table row from anything array-like of non-negative integers; Error otherwise."""
    m = np.ascontiguousarray(m)
    if m.dtype != np.uint32:
        if m.size and (np.any(m < 0) or np.any(m > 0xFFFFFFFF) or np.any(m != np.floor(m))):
            raise Error("sample multiplicities are integers in [0, 2^32 - 1]")
        m = m.astype(np.uint32)
    return m.reshape(-1)


def kde_weighted_bandwidths(samples, nfields, nobservables, lower, upper, bandwidth_scale, multiplicities=None):
    """sxmc_kde_weighted_bandwidths: the bandwidth law of an EvalKernel over weighted samples on the host alone (no
    device is touched).  Returns a dict of h, sigma, mean (float64 [nobservables]), n_eff, s1, s2; raises Error where
    the constructor would."""
    samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    lower = np.ascontiguousarray(lower, dtype=np.float64)
    upper = np.ascontiguousarray(upper, dtype=np.float64)
    scale = np.ascontiguousarray(bandwidth_scale, dtype=np.float64).reshape(-1)
    m = None if multiplicities is None else _multiplicities(multiplicities)
    D = max(int(nobservables), 0)
    h, sigma, mean = np.zeros(D), np.zeros(D), np.zeros(D)
    n_eff, s1, s2 = C.c_double(0), C.c_double(0), C.c_double(0)
    _raise(capi.load().sxmc_kde_weighted_bandwidths(
        capi.ptr(samples), samples.size, int(nfields), int(nobservables), capi.ptr(lower), lower.size, capi.ptr(upper),
        upper.size, capi.ptr(scale), scale.size, capi.ptr(m), 0 if m is None else m.size, capi.ptr(h), capi.ptr(sigma),
        capi.ptr(mean), C.byref(n_eff), C.byref(s1), C.byref(s2)))
    return {"h": h, "sigma": sigma, "mean": mean, "n_eff": n_eff.value, "s1": s1.value, "s2": s2.value}


class CvOptions:
    """The grid and the search of EvalKernel's cross-validation (sxmc_amd/csrc/kde_cv.h): multipliers
    lo (hi/lo)^(k/(steps-1)) of Scott's rule, a common scan and (per_observable) one coordinate scan per observable,
    on at most max_rows rows (0: all)."""

    def __init__(self, lo=0.125, hi=4.0, steps=21, per_observable=True, max_rows=65536):
        self.lo, self.hi, self.steps = float(lo), float(hi), int(steps)
        self.per_observable, self.max_rows = bool(per_observable), int(max_rows)

    def __eq__(self, other):
        return isinstance(other, CvOptions) and vars(self) == vars(other)

    def __repr__(self):
        return "CvOptions(lo=%r, hi=%r, steps=%d, per_observable=%r, max_rows=%d)" % (
            self.lo, self.hi, self.steps, self.per_observable, self.max_rows)


class CvScan:
    """One scan of a search: observable -1 is the common multiplier on all observables."""

    def __init__(self, observable, grid, scores, chosen):
        self.observable, self.grid, self.scores, self.chosen = int(observable), grid, scores, int(chosen)


class CvReport:
    """What a search chose: `scale` (a bandwidth_scale), its `score`, `score_at_one` (NaN when 1 is not on the
    grid), every scan, `at_edge[d]` when observable d's choice sits on the first or last grid value, `rows_used`."""

    def __init__(self, scale, score, score_at_one, scans, at_edge, rows_used):
        self.scale = np.asarray(scale, dtype=np.float64)
        self.score, self.score_at_one = float(score), float(score_at_one)
        self.scans, self.at_edge, self.rows_used = list(scans), list(at_edge), int(rows_used)


class EvalKernel(_Eval):
    """pdfz::EvalKernel (pdfz.h:578-625): the kernel-density PDF, contract in sxmc_amd/include/sxmc/pdfz.h.
    Same method names as EvalHist (RandomSample and Shared included), plus Bandwidths(); at most 4 observables;
    O(points x samples) per evaluation.  bandwidth_sensitivity in [0, 1] (alpha) turns on Abramson's adaptive
    bandwidths h_d * lambda_i, lambda_i fixed per table row at construction (LocalFactors()); 0.0, the default, is the
    fixed-bandwidth evaluator, the same kernels and bits as before the keyword existed.
    multiplicities (one non-negative integer per table row, host memory; None: none) makes it an evaluator over
    weighted Monte Carlo samples (sxmc_kde_create_weighted, the laws in include/sxmc_hip.h): given here, never set
    afterwards; SampleTotal(), SampleMultiplicities() and EffectiveSamples() read them back.  Cross-validation of such
    an evaluator is refused."""

    _prefix = "sxmc_kde_"

    def __init__(self, samples, nfields, nobservables, lower, upper, bandwidth_scale, dataset=0,
                 bandwidth_sensitivity=0.0, multiplicities=None):
        scale = np.ascontiguousarray(bandwidth_scale, dtype=np.float64).reshape(-1)
        alpha = float(bandwidth_sensitivity)
        lib = capi.load()
        if multiplicities is not None:
            m = _multiplicities(multiplicities)

            def create(*a):
                return lib.sxmc_kde_create_weighted(*a[:-1], alpha, capi.ptr(m), m.size, a[-1])
        elif alpha == 0.0:
            create = lib.sxmc_kde_create
        else:
            def create(*a):
                return lib.sxmc_kde_create_adaptive(*a[:-1], alpha, a[-1])
        self._create(create, samples, nfields, nobservables, lower, upper, scale, dataset)

    def SampleTotal(self):
        """The multiplicities' total, or the row count when none are set: n_mc for either kind."""
        return self._get("sample_total", C.c_ulonglong)

    def SampleMultiplicities(self):
        """The multiplicities (uint32 [nsamples]); all 1 when none are set."""
        out = np.empty(self.nsamples, dtype=np.uint32)
        self._call("get_sample_multiplicities", capi.ptr(out), out.size, None)
        return out

    def HasSampleMultiplicities(self):
        is_set = C.c_int(0)
        self._call("get_sample_multiplicities", None, 0, C.byref(is_set))
        return bool(is_set.value)

    def EffectiveSamples(self):
        """Kish's n_eff = (sum m)^2 / sum m^2 over the in-domain rows, which stands where n stood in the bandwidth rule;
        the in-domain row count when no multiplicities are set."""
        return self._get("effective_samples", C.c_double)

    @classmethod
    def CrossValidated(cls, samples, nfields, nobservables, lower, upper, options=None, dataset=0,
                       bandwidth_sensitivity=0.0):
        """An evaluator whose bandwidth scales are chosen by leave-one-out likelihood cross-validation
        (sxmc_kde_cv_select, contract in include/sxmc_hip.h): a provisional fixed-bandwidth evaluator at scale 1 runs
        the search, then the evaluator is built with the chosen scales and the asked sensitivity, exactly as if the
        scales had been typed in.  CvReport() is the search's report."""
        pilot = cls(samples, nfields, nobservables, lower, upper, np.ones(int(nobservables)), dataset)
        try:
            report = pilot.SelectBandwidthScale(options)
        finally:
            pilot.close()
        self = cls(samples, nfields, nobservables, lower, upper, report.scale, dataset, bandwidth_sensitivity)
        self._cv_report = report
        return self

    @classmethod
    def Shared(cls, base):
        self = super().Shared(base)
        self._cv_report = getattr(base, "_cv_report", None)
        return self

    def CvScores(self, candidates, max_rows=0):
        """score(h) of each absolute candidate bandwidth vector (rows of `candidates`, at most 32) on this evaluator's
        table, and the rows scored: (float64 [K], m).  No search (sxmc_kde_cv_scores)."""
        cand = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, self.nobservables)
        scores = np.empty(cand.shape[0], dtype=np.float64)
        m = C.c_size_t(0)
        self._call("cv_scores", capi.ptr(cand), cand.shape[0], int(max_rows), capi.ptr(scores), C.byref(m))
        return scores, m.value

    def SelectBandwidthScale(self, options=None):
        """The search of sxmc_kde_cv_select on this evaluator's table: a CvReport whose `scale` is a bandwidth_scale.
        The evaluator's own bandwidths do not change."""
        o = options if options is not None else CvOptions()
        D, steps = self.nobservables, int(o.steps)
        room = (1 + D) * max(steps, 1)
        scale = np.zeros(D)
        score, at_one = C.c_double(0), C.c_double(0)
        at_edge = np.zeros(D, dtype=np.int32)
        rows, nscans = C.c_size_t(0), C.c_int(0)
        grid, scores = np.zeros(room), np.zeros(room)
        chosen = np.zeros(1 + D, dtype=np.int32)
        self._call("cv_select", float(o.lo), float(o.hi), steps, int(bool(o.per_observable)), int(o.max_rows),
                   capi.ptr(scale), D, C.byref(score), C.byref(at_one), capi.ptr(at_edge), C.byref(rows),
                   C.byref(nscans), capi.ptr(grid), capi.ptr(scores), capi.ptr(chosen))
        scans = [CvScan(s - 1, grid[s * steps:(s + 1) * steps].copy(), scores[s * steps:(s + 1) * steps].copy(),
                        int(chosen[s])) for s in range(nscans.value)]
        return CvReport(scale, score.value, at_one.value, scans, [bool(e) for e in at_edge], rows.value)

    def BandwidthScale(self):
        """The bandwidth scales the evaluator was constructed with: typed in, or chosen by CrossValidated."""
        out = np.empty(self.nobservables, dtype=np.float64)
        self._call("bandwidth_scale", capi.ptr(out), out.size)
        return out

    def CvReport(self):
        """The report of the search behind CrossValidated (a shared evaluator: its base's); None otherwise."""
        return getattr(self, "_cv_report", None)

    def BandwidthSensitivity(self):
        """The alpha the evaluator was constructed with (a shared evaluator: its base's)."""
        return self._get("sensitivity", C.c_double)

    def LocalFactors(self):
        """lambda_i of every table row, fixed at construction (float64 [nsamples]); all 1.0 at sensitivity 0."""
        out = np.empty(self.nsamples, dtype=np.float64)
        self._call("local_factors", capi.ptr(out), out.size)
        return out

    def SetCutoff(self, R):
        """A cutoff radius on the pair sum in units of each sample's own bandwidth (sxmc_kde_set_cutoff, contract in
        include/sxmc_hip.h): 0 turns it off (the evaluator as it was, bit for bit), 1 <= R <= inf drops pairs at least
        R bandwidths apart, a 256-sample tile against a wave of 64 points at a time.  The evaluator must be idle."""
        self._call("set_cutoff", float(R))

    def Cutoff(self):
        """R (a shared evaluator: its base's when it was made)."""
        return self._get("cutoff", C.c_double)

    def CutoffStats(self):
        """(tiles_visited, tiles_possible) of the last evaluation; (0, 0) when it ran without a cutoff or a lookup."""
        visited, possible = C.c_ulonglong(0), C.c_ulonglong(0)
        self._call("cutoff_stats", C.byref(visited), C.byref(possible))
        return visited.value, possible.value

    def CutoffBoxes(self):
        """(tile boxes [tiles, 9], wave boxes [waves, 8]) as float32: lo[4], hi[4] (and a tile's smallest g) of the
        last evaluation's sorted sample tiles and of the point plan's waves (sxmc_kde_cutoff_boxes; for tests)."""
        ntiles = max(1, -(-self.nsamples // 256))
        nwaves = max(256, -(-self.npoints // 256) * 256) // 64
        tiles, waves = np.zeros((ntiles, 9), np.float32), np.zeros((nwaves, 8), np.float32)
        self._call("cutoff_boxes", capi.ptr(tiles), tiles.size, capi.ptr(waves), waves.size)
        return tiles, waves

    def PairSplit(self):
        """(nsplit, tiles_per_split) of the current point plan: the workgroups to every 256 points of the pair sum's
        next launch and the 256-row sample tiles each walks (sxmc_kde_pair_split; for tests).  Launches nothing."""
        nsplit, tps = C.c_int(0), C.c_uint(0)
        self._call("pair_split", C.byref(nsplit), C.byref(tps))
        return nsplit.value, tps.value

    def Bandwidths(self):
        """h_d = bandwidth_scale_d * sigma_d * n^(-1/(D+4)) (Scott's rule), fixed at construction."""
        out = np.empty(self.nobservables, dtype=np.float64)
        self._call("bandwidths", capi.ptr(out), out.size)
        return out

    def EvalOnStream(self, stream, do_eval_pdf=True):
        """EvalAsync's launches on the caller's stream (sxmc_kde_eval_on_stream_async): same kernels, same bits,
        capture-safe; the evaluator orders its other calls after the last work given to that stream."""
        self._call("eval_on_stream_async", int(bool(do_eval_pdf)), capi.ptr(stream))

    def ParametersRead(self):
        """The parameter indices the attached systematics read (int16), before the parameter buffer's offset."""
        n = C.c_size_t(0)
        self._call("parameters_read", None, 0, C.byref(n))
        out = np.zeros(n.value, dtype=np.int16)
        self._call("parameters_read", capi.ptr(out), out.size, C.byref(n))
        return out

    def EvaluationCount(self):
        """Evaluations launched so far, by EvalAsync or EvalOnStream (for tests and reports)."""
        return self._get("evaluation_count", C.c_ulonglong)

    def SamplePool(self):
        """How many samples the last evaluation left inside the domain, as the sampler counts them (= the norm)."""
        return self._get("sample_pool", C.c_size_t)

    def Project(self, obs, nbins):
        """sxmc_kde_project: per bin the analytic integral of every in-domain sample's truncated Gaussian, in f64."""
        out = np.zeros(max(int(nbins), 0), dtype=np.float64)
        self._call("project", int(obs), int(nbins), capi.ptr(out))
        return out
