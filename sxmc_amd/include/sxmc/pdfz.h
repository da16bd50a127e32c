// pdfz.h -- the reference's pdfz interface (src/pdfz.h:87-627) on MI355X.
//
// Same names, constructor arguments, defaults, virtuals and throw behaviour as pdfz::Eval /
// pdfz::EvalHist / pdfz::EvalKernel, so that callers written against the reference (mcmc.cpp:233-242, 264-271,
// signal.cpp:131-146, 192-196, bench_sxmc.cpp:58-96) compile against this header.  Everything is a
// thin layer over the C ABI of libsxmc_hip.so (include/sxmc_hip.h); the arithmetic runs in
// hand-written gfx950 kernels.  Differences, all forced by what is absent here:
//   * ROOT-returning methods (CreateHistogram, CreateHistogramProjection, DefaultHistogram,
//     RandomSample) are replaced by plain-array accessors (GetBins, GetNormalizedHistogram, Project, SampleEvents);
//   * Optimize/OptimizeBin/OptimizeEval (brute-force launch autotuning, pdfz.cpp:622-814): the constructor's
//     `optimize` flag and Optimize() keep their meaning -- trial launches at the first evaluation with evaluation
//     points -- but the trials are those of the BATCH the library forms behind the per-evaluator calls
//     (sxmc_hist_set_optimize, include/sxmc_hip.h); the lookup's launch shape has nothing to choose;
//   * a systematic's parameter-index array is read when AddSystematic is called (the reference keeps
//     the pointer and reads it at every evaluation, pdfz.cpp:143).
#pragma once

#include <string>
#include <vector>

#include "device_array.h"

#ifndef SXMC_ARRAY_TEMPLATE
#define SXMC_ARRAY_TEMPLATE sxmc::DeviceArray
#endif

namespace pdfz {

template <typename T>
using Array = SXMC_ARRAY_TEMPLATE<T>;

/** pdfz::Error (pdfz.h:93-102): thrown by value. */
struct Error {
  Error(const std::string& _msg) { msg = _msg; }
  std::string msg;
};

/** pdfz::Systematic and its four kinds (pdfz.h:109-233). */
struct Systematic {
  enum Type { SHIFT, SCALE, RESOLUTION_SCALE, CTSCALE };
  Type type;
  Systematic(Type _type) : type(_type) {}
  virtual ~Systematic() {}
};

struct ShiftSystematic : public Systematic {  // x' = x + p
  ShiftSystematic(int _obs, Array<short>* _pars) : Systematic(SHIFT), obs(_obs), pars(_pars) {}
  int obs;
  Array<short>* pars;
};

struct ScaleSystematic : public Systematic {  // x' = x * (1 + p)
  ScaleSystematic(int _obs, Array<short>* _pars) : Systematic(SCALE), obs(_obs), pars(_pars) {}
  int obs;
  Array<short>* pars;
};

struct CosThetaScaleSystematic : public Systematic {  // x' = 1 + (x - 1) * (1 + p)
  CosThetaScaleSystematic(int _obs, Array<short>* _pars) : Systematic(CTSCALE), obs(_obs), pars(_pars) {}
  int obs;
  Array<short>* pars;
};

struct ResolutionScaleSystematic : public Systematic {  // x' = x + p * (x - x_true)
  ResolutionScaleSystematic(int _obs, int _true_obs, Array<short>* _pars)
      : Systematic(RESOLUTION_SCALE), obs(_obs), true_obs(_true_obs), pars(_pars) {}
  int obs;
  int true_obs;
  Array<short>* pars;
};

inline void throw_on(int rc) {
  if (rc == SXMC_OK) return;
  if (rc == SXMC_ERR_INVALID) throw Error(sxmc_last_error());
  throw sxmc::HipError(std::string("libsxmc_hip: ") + sxmc_last_error());
}

/** pdfz::Eval (pdfz.h:246-395): abstract evaluator interface. */
class Eval {
 public:
  /** Same arguments as the reference (pdfz.h:268-270).  The size validation of pdfz.cpp:64-82 is
   *  performed, in the same order and with the same messages, by sxmc_hist_create. */
  Eval(const std::vector<float>& /*samples*/, int _nfields, int _nobservables,
       const std::vector<double>& /*lower*/, const std::vector<double>& /*upper*/, unsigned _dataset = 0)
      : nfields(_nfields), nobservables(_nobservables), dataset(_dataset) {}
  virtual ~Eval() {}

 protected:
  Eval(int _nfields, int _nobservables, unsigned _dataset)
      : nfields(_nfields), nobservables(_nobservables), dataset(_dataset) {}

 public:
  virtual void SetEvalPoints(const std::vector<float>& points) = 0;
  virtual void SetPDFValueBuffer(Array<float>* output, int offset = 0, int stride = 1) {
    pdf_buffer = output;
    pdf_offset = offset;
    pdf_stride = stride;
  }
  virtual void SetNormalizationBuffer(Array<unsigned int>* norm, int offset = 0) {
    norm_buffer = norm;
    norm_offset = offset;
  }
  virtual void SetParameterBuffer(Array<double>* params, int offset = 0, int stride = 1) {
    param_buffer = params;
    param_offset = offset;
    param_stride = stride;
  }
  virtual void AddSystematic(const Systematic& syst) = 0;
  virtual void EvalAsync(bool do_eval_pdf = true) = 0;
  virtual void EvalFinished() = 0;
  /** The three buffers are BORROWED (pdfz.cpp:106-124 stores raw pointers, like this class): a caller whose
   *  buffers are about to die un-binds them, so that the next evaluation binds afresh or fails loudly instead of
   *  touching destroyed arrays.  (The reference leaves the dangling pointers in place.) */
  virtual void ForgetBuffers() {
    pdf_buffer = nullptr;
    norm_buffer = nullptr;
    param_buffer = nullptr;
  }
  /** The sampling step of RandomSample (pdfz.cpp:843-918) on the device: appends `observed` events (rows of
   *  nobservables + 1 floats, last = dataset id) drawn from the PDF of the last evaluation -- a histogram's bins
   *  (EvalAsync(false) first, as CreateHistogram does) or a kernel-density PDF's moved samples -- redrawn while
   *  outside [lowers, uppers] when given. */
  virtual void SampleEvents(std::vector<float>& events, size_t observed, unsigned long long seed,
                            const std::vector<float>& uppers = std::vector<float>(),
                            const std::vector<float>& lowers = std::vector<float>()) = 0;
  /** A new evaluator of the same kind over the SAME sample table (the SharedSamples constructors); the caller
   *  deletes it. */
  virtual Eval* Share() const = 0;
  /** The share of the PDF of the last evaluation in each of `nbins` equal bins of observable `obs` (what
   *  CreateHistogramProjection, pdfz.h:505-518, hands to plot_fit, normalised): the shares sum to 1, or are all 0 when
   *  the norm is 0.  Computed on the device; the evaluation's results stay as they are. */
  virtual std::vector<double> Project(int /*obs*/, int /*nbins*/) {
    throw Error("Project is not implemented by this evaluator");
  }

  /** The data set the evaluator's points are looked up for (the constructor's `dataset`). */
  unsigned Dataset() const { return dataset; }

 protected:
  int nfields;
  int nobservables;
  unsigned dataset;
  Array<float>* pdf_buffer = nullptr;
  int pdf_offset = 0;
  int pdf_stride = 1;
  Array<unsigned int>* norm_buffer = nullptr;
  int norm_offset = 0;
  Array<double>* param_buffer = nullptr;
  int param_offset = 0;
  int param_stride = 1;
};

namespace detail {

/** A systematic of any of the four kinds as sxmc_*_add_systematic takes it. */
struct SystematicFields {
  int type, obs, extra;
  Array<short>* pars;
};
inline SystematicFields unpack(const Systematic& syst) {
  switch (syst.type) {
    case Systematic::SHIFT: {
      const ShiftSystematic& s = dynamic_cast<const ShiftSystematic&>(syst);
      return {syst.type, s.obs, 0, s.pars};
    }
    case Systematic::SCALE: {
      const ScaleSystematic& s = dynamic_cast<const ScaleSystematic&>(syst);
      return {syst.type, s.obs, 0, s.pars};
    }
    case Systematic::CTSCALE: {
      const CosThetaScaleSystematic& s = dynamic_cast<const CosThetaScaleSystematic&>(syst);
      return {syst.type, s.obs, 0, s.pars};
    }
    case Systematic::RESOLUTION_SCALE: {
      const ResolutionScaleSystematic& s = dynamic_cast<const ResolutionScaleSystematic&>(syst);
      return {syst.type, s.obs, s.true_obs, s.pars};
    }
  }
  throw Error("Unknown systematic type");
}

/** Tag of the sharing constructors: EvalHist(base, SharedSamples{}), EvalKernel(base, SharedSamples{}). */
struct SharedSamples {};

/** The entry points of include/sxmc_hip.h that the two families of evaluators have in common. */
struct HistApi {
  typedef sxmc_hist_t Handle;
  static constexpr auto create_shared = sxmc_hist_create_shared;
  static constexpr auto destroy = sxmc_hist_destroy;
  static constexpr auto set_eval_points = sxmc_hist_set_eval_points;
  static constexpr auto add_systematic = sxmc_hist_add_systematic;
  static constexpr auto set_pdf_value_buffer = sxmc_hist_set_pdf_value_buffer;
  static constexpr auto set_normalization_buffer = sxmc_hist_set_normalization_buffer;
  static constexpr auto set_parameter_buffer = sxmc_hist_set_parameter_buffer;
  static constexpr auto eval_async = sxmc_hist_eval_async;
  static constexpr auto eval_finished = sxmc_hist_eval_finished;
  static constexpr auto random_sample = sxmc_hist_random_sample;
};
struct KernelApi {
  typedef sxmc_kde_t Handle;
  static constexpr auto create_shared = sxmc_kde_create_shared;
  static constexpr auto destroy = sxmc_kde_destroy;
  static constexpr auto set_eval_points = sxmc_kde_set_eval_points;
  static constexpr auto add_systematic = sxmc_kde_add_systematic;
  static constexpr auto set_pdf_value_buffer = sxmc_kde_set_pdf_value_buffer;
  static constexpr auto set_normalization_buffer = sxmc_kde_set_normalization_buffer;
  static constexpr auto set_parameter_buffer = sxmc_kde_set_parameter_buffer;
  static constexpr auto eval_async = sxmc_kde_eval_async;
  static constexpr auto eval_finished = sxmc_kde_eval_finished;
  static constexpr auto random_sample = sxmc_kde_random_sample;
};

/** What EvalHist and EvalKernel share: an evaluator of the library behind a handle, driven through Api's entry
 *  points.  The concrete class's constructor creates the handle. */
template <class Api>
class EvalOver : public Eval {
 public:
  typedef detail::SharedSamples SharedSamples;
  EvalOver(const EvalOver&) = delete;
  EvalOver& operator=(const EvalOver&) = delete;
  virtual ~EvalOver() { Api::destroy(handle); }

  virtual void SetEvalPoints(const std::vector<float>& points) {
    throw_on(Api::set_eval_points(handle, points.data(), points.size()));
  }

  virtual void AddSystematic(const Systematic& syst) {
    const SystematicFields f = unpack(syst);
    throw_on(Api::add_systematic(handle, f.type, f.obs, f.extra, (int)f.pars->size(), f.pars->readOnlyHostPtr()));
  }

  /** Bind the three caller buffers (device side) and launch the evaluation on this evaluator's stream -- zero + fill
   *  (+ lookup) for a histogram (pdfz.cpp:441-488), prepass (+ pair sum + combine) for a kernel density; returns
   *  before completion. */
  virtual void EvalAsync(bool do_eval_pdf = true) {
    Bind();
    throw_on(Api::eval_async(handle, do_eval_pdf ? 1 : 0));
  }
  virtual void EvalFinished() { throw_on(Api::eval_finished(handle)); }

  void ForgetBuffers() override {
    Eval::ForgetBuffers();
    throw_on(Api::set_pdf_value_buffer(handle, nullptr, 0, 1));
    throw_on(Api::set_normalization_buffer(handle, nullptr, 0));
    throw_on(Api::set_parameter_buffer(handle, nullptr, 0, 1));
  }

  /** The accessor calls of pdfz.cpp:457-470, 484-487: outputs become device-valid (host copies are
   *  stale until read back), parameters are uploaded if the host side is newer. */
  void Bind() {
    if (pdf_buffer) throw_on(Api::set_pdf_value_buffer(handle, pdf_buffer->writeOnlyPtr(), pdf_offset, pdf_stride));
    if (norm_buffer) throw_on(Api::set_normalization_buffer(handle, norm_buffer->writeOnlyPtr(), norm_offset));
    if (param_buffer) throw_on(Api::set_parameter_buffer(handle, param_buffer->readOnlyPtr(), param_offset, param_stride));
  }

  void SampleEvents(std::vector<float>& events, size_t observed, unsigned long long seed,
                    const std::vector<float>& uppers = std::vector<float>(),
                    const std::vector<float>& lowers = std::vector<float>()) override {
    const size_t row = (size_t)nobservables + 1, old = events.size();
    events.resize(old + observed * row);
    const bool cuts = !uppers.empty() && !lowers.empty();
    throw_on(Api::random_sample(handle, observed, seed, cuts ? lowers.data() : nullptr,
                                cuts ? uppers.data() : nullptr, events.data() + old));
  }

  typename Api::Handle Handle() const { return handle; }

 protected:
  EvalOver(int _nfields, int _nobservables, unsigned _dataset) : Eval(_nfields, _nobservables, _dataset) {}
  /** A second evaluator over the SAME sample table as `base` (nothing copied; own histogram or rows, event bins or
   *  points, bindings and stream; systematics as attached to `base` so far): one per concurrent chain on a GPU. */
  EvalOver(const EvalOver& base, SharedSamples) : Eval(base.nfields, base.nobservables, base.dataset) {
    throw_on(Api::create_shared(base.handle, &handle));
  }
  typename Api::Handle handle = nullptr;
};

}  // namespace detail

/** pdfz::EvalHist (pdfz.h:402-574): N-dimensional histogram PDF. */
class EvalHist : public detail::EvalOver<detail::HistApi> {
 public:
  EvalHist(const std::vector<float>& samples, int nfields, int nobservables, const std::vector<double>& lower,
           const std::vector<double>& upper, const std::vector<int>& nbins, unsigned dataset = 0,
           bool optimize = true)
      : EvalOver(nfields, nobservables, dataset) {
    throw_on(sxmc_hist_create(samples.data(), samples.size(), 0, nfields, nobservables, lower.data(),
                              lower.size(), upper.data(), upper.size(), nbins.data(), nbins.size(), dataset,
                              &handle));
    throw_on(sxmc_hist_set_optimize(handle, optimize ? 1 : 0));   // needs_optimization(optimize), pdfz.cpp:188
    axis_nbins = nbins;
  }
  EvalHist(const EvalHist& base, SharedSamples s) : EvalOver(base, s), axis_nbins(base.axis_nbins) {}
  Eval* Share() const override { return new EvalHist(*this, SharedSamples{}); }

  /** pdfz.cpp:622-628: trial launches choose the launch shape -- here at the next lookup evaluation of the batch this
   *  evaluator is evaluated in (they need an evaluation's bindings).  OptimizeBin (:630-727) is that choice for the fill;
   *  OptimizeEval (:729-814) tuned the lookup kernel, whose shape is one lane per evaluation point here: nothing to try. */
  virtual void Optimize() { throw_on(sxmc_hist_optimize(handle)); }
  virtual void OptimizeBin() { throw_on(sxmc_hist_optimize(handle)); }
  virtual void OptimizeEval() {}

  /** The launch plan of the batch this evaluator's evaluations run in + "tuned=.. trial_launches=.." (tests, logs). */
  std::string LaunchInfo() {
    std::vector<char> buf(16384);
    throw_on(sxmc_hist_launch_info(handle, buf.data(), buf.size()));
    return std::string(buf.data());
  }

  /** WEIGHTED MONTE CARLO SAMPLES: one integer multiplicity per table row; the fill adds m_i where it added 1
   *  (include/sxmc_hip.h, sxmc_hist_set_sample_multiplicities: the law).  Before the first evaluation and before the
   *  evaluator joins a group (an MCMC, an ensemble); a total beyond 2^32 - 1 throws.  Share() shares the column. */
  void SetSampleMultiplicities(const std::vector<unsigned>& m) {
    throw_on(sxmc_hist_set_sample_multiplicities(handle, m.data(), m.size(), 0));
  }
  /** The multiplicities' total, or the row count when none are set: what n_mc is for either kind. */
  unsigned long long SampleTotal() {
    unsigned long long total = 0;
    throw_on(sxmc_hist_sample_total(handle, &total));
    return total;
  }
  bool HasSampleMultiplicities() {
    int is_set = 0;
    throw_on(sxmc_hist_get_sample_multiplicities(handle, nullptr, 0, &is_set));
    return is_set != 0;
  }
  /** The multiplicities; all 1 when none are set. */
  std::vector<unsigned> SampleMultiplicities() {
    size_t n = 0;
    throw_on(sxmc_hist_nsamples(handle, &n));
    std::vector<unsigned> out(n);
    throw_on(sxmc_hist_get_sample_multiplicities(handle, out.data(), out.size(), nullptr));
    return out;
  }

  /** pdfz.h:542-556 */
  void GetSamples(std::vector<float>& sv) {
    size_t n = 0;
    throw_on(sxmc_hist_nsamples(handle, &n));
    const size_t oldsize = sv.size();
    sv.resize(oldsize + n * (size_t)(nobservables + 1));
    throw_on(sxmc_hist_get_samples(handle, sv.data() + oldsize, n * (size_t)(nobservables + 1)));
  }

  /** Bin contents of the last evaluation, row-major (what CreateHistogram reads, pdfz.cpp:511). */
  std::vector<unsigned> GetBins() {
    int b = 0;
    throw_on(sxmc_hist_total_nbins(handle, &b));
    std::vector<unsigned> out((size_t)b);
    throw_on(sxmc_hist_get_bins(handle, out.data(), out.size()));
    return out;
  }

  /** The bins of the last evaluation summed over every observable but `obs`, on the device (sxmc_hist_project): exact
   *  integers, and only the marginal is copied to the host. */
  std::vector<unsigned long long> ProjectCounts(int obs) {
    if (obs < 0 || obs >= nobservables) throw Error("no such observable to project onto");
    std::vector<unsigned long long> out((size_t)axis_nbins[(size_t)obs], 0ull);
    throw_on(sxmc_hist_project(handle, obs, out.data(), out.size()));
    return out;
  }

  /** counts / sum of counts along `obs`; nbins must be the evaluator's own bin count there. */
  std::vector<double> Project(int obs, int nbins) override {
    if (obs < 0 || obs >= nobservables || nbins != axis_nbins[(size_t)obs]) {
      throw Error("EvalHist projects onto its own bins: " + std::to_string(nbins) + " asked along observable " +
                  std::to_string(obs));
    }
    const std::vector<unsigned long long> counts = ProjectCounts(obs);
    unsigned long long total = 0;
    for (unsigned long long c : counts) total += c;
    std::vector<double> out(counts.size(), 0.0);
    if (total > 0)
      for (size_t j = 0; j < counts.size(); j++) out[j] = (double)counts[j] / (double)total;
    return out;
  }

  /** ROOT-free CreateHistogram (pdfz.cpp:498-594): fill only (EvalAsync(false)), then
   *  content = bins / bin_volume / norm, or 0 when norm == 0; row-major. */
  std::vector<double> GetNormalizedHistogram() {
    EvalAsync(false);
    EvalFinished();
    std::vector<unsigned> bins = GetBins();
    const unsigned norm = norm_buffer->readOnlyHostPtr()[norm_offset];
    double vol = 0;
    throw_on(sxmc_hist_bin_volume(handle, &vol));
    std::vector<double> out(bins.size(), 0.0);
    if (norm > 0)
      for (size_t i = 0; i < bins.size(); i++) out[i] = bins[i] / vol / norm;
    return out;
  }

 protected:
  std::vector<int> axis_nbins;   //!< bins per observable, as constructed
};

/** pdfz::EvalKernel::CvOptions, the grid and the search of its cross-validation: multipliers lo (hi/lo)^(k/(steps-1)) of Scott's rule, a common scan
 *  and (per_observable) one coordinate scan per observable, on at most max_rows rows (0: all). */
struct KernelCvOptions {
  double lo = 0.125, hi = 4.0;
  int steps = 21;
  bool per_observable = true;
  size_t max_rows = 65536;
};
/** pdfz::EvalKernel::CvScan, one scan of a search; observable -1 is the common multiplier on all observables. */
struct KernelCvScan {
  int observable = -1;
  std::vector<double> grid, scores;
  int chosen = -1;
};
/** pdfz::EvalKernel::CvResult, what a search chose. */
struct KernelCvResult {
  std::vector<double> scale;   //!< the chosen multipliers of Scott's rule: a bandwidth_scale
  double score = 0.0;          //!< the score of the choice
  double score_at_one = 0.0;   //!< the common scan's score at s = 1; NaN when 1 is not on the grid
  std::vector<KernelCvScan> scans;   //!< the common scan, then one per observable
  std::vector<int> at_edge;    //!< per observable: the choice sits on the first or last grid value
  size_t rows_used = 0;        //!< m
};

/** pdfz::EvalKernel (pdfz.h:578-625; declared by the reference, implemented here): the kernel-density PDF, the unbinned
 *  alternative to EvalHist for signals whose Monte Carlo sample is too small to fill a fine histogram.
 *
 *  Constructor: (samples, nfields, nobservables, lower, upper, bandwidth_scale) as the reference declares it, plus
 *  the optional `dataset` EvalHist has.  Validation needs no GPU: Eval::Eval's checks with the reference's messages in
 *  its order (pdfz.cpp:64-82), then "Number of bandwidth scales must be same as number of observables.", the
 *  MAX_NFIELDS check, at most 4 observables (this class's limit), every scale positive and finite, upper > lower.
 *  Bandwidths (Scott's rule), fixed at construction and computed on the host in f64:
 *    h_d = bandwidth_scale_d * sigma_d * n^(-1/(D+4)), sigma_d the sample standard deviation (n - 1) of observable d
 *    over the n untransformed samples whose observables all lie in [lower, upper); n < 2 or a zero sigma throws.
 *  Per evaluation:
 *    - every attached systematic moves every sample, with the f64 arithmetic of EvalHist's fill;
 *    - a sample is in the domain when lower <= x < upper for every observable (NaN is outside); norm = their count,
 *      written to the normalization buffer: EvalHist's norm on the same inputs, bit for bit;
 *    - an in-domain sample s_i carries w_i = 1 / prod_d [Phi((upper_d - s_id)/h_d) - Phi((lower_d - s_id)/h_d)], the
 *      kernel truncated to the domain and renormalised; the others weigh 0;
 *    - pdf(x) = (1/norm) sum_i w_i prod_d phi((x_d - s_id)/h_d)/h_d, whose integral over the domain is 1;
 *    - points as EvalHist::SetEvalPoints: any observable outside the domain NaN (whatever the data set), inside and
 *      of another data set 0, norm == 0 NaN; values go as float to pdf_out[offset + stride * i];
 *    - EvalAsync(false) computes the norm only.  EvalAsync returns before completion, EvalFinished waits.
 *  Deterministic: the same inputs give the same bits (no floating-point atomics).  Cost O(points x samples).
 *  Accuracy: a value's relative error is at most about 2^-24 (128 + 2.8 c_max), c_max the largest (x - lower) / h over
 *  the points and samples (f32 coordinates measured from lower, f32 sums over 256-sample tiles): measured 2e-6 at
 *  c_max ~ 20, 1e-5 at ~ 100 and 9e-5 at ~ 900 (tests/kde_reference.py has the bound, tests/test_gpu_kde_dims.py).
 *  Fake data: SampleEvents draws from the PDF of the last evaluation (EvalAsync(false) or (true) first): a moved
 *  in-domain sample chosen uniformly, then per observable its Gaussian truncated to [lower, upper); every event passes
 *  the domain test above.  Counter-based (Philox4x32-10 keyed by the seed): the same seed gives the same events.
 *  Concurrent experiments: EvalKernel(base, SharedSamples{}) shares base's sample table (systematics, bandwidths
 *  copied; own rows, points, bindings and stream) and may outlive it.
 *
 *  Adaptive (sample-point) bandwidths, Abramson's estimator (Silverman 5.3): the last constructor argument, the
 *  bandwidth sensitivity alpha in [0, 1] (anything else, or not finite, throws).  alpha = 0, the default, is everything
 *  above: the same kernels, the same row layout, the same bits.  For alpha > 0 every table row i gets a factor lambda_i
 *  on all its bandwidths, fixed at construction on the UNTRANSFORMED table, after the Scott bandwidths h_d:
 *    pilot    S0 = the n untransformed samples inside the domain.  For every table row i (inside or not), in f64:
 *               f_i = (1/n) sum_{j in S0} w_j prod_d phi((x_id - x_jd)/h_d)/h_d,
 *               w_j = 1 / prod_d [Phi((upper_d - x_jd)/h_d) - Phi((lower_d - x_jd)/h_d)],
 *             this evaluator's own fixed-bandwidth PDF at zero systematics, taken at the sample; the same formula
 *             continues outside the domain.  The difference x_id - x_jd is taken first, on the f64 values of the
 *             floats, then divided by h_d; Phi through erfc, as the prepass writes it.
 *    scale    g = exp((1/n) sum_{i in S0} ln f_i), on the host in f64, in table order; f_i > 0 on S0 because a row's
 *             own term is positive.
 *    factors  lambda_i = min(10, max(0.1, (f_i/g)^(-alpha))); a row whose f_i is not finite and positive takes 10.  The
 *             clips bound how far the f32 coordinates of the pair sum are stretched.
 *  The factors belong to table rows: a sample keeps its lambda_i wherever the systematics move it, rows that start
 *  outside the domain and move in included.  Per evaluation, s_i the moved samples, norm the in-domain count (unchanged):
 *    pdf(x) = (1/norm) sum_{i in domain} w_i prod_d phi((x_d - s_id)/(h_d lambda_i))/(h_d lambda_i),
 *    w_i the truncation weight at bandwidth h_d lambda_i: the integral over the domain is still exactly 1.  Point
 *    codes, the NaN / 0 rules and norm = 0 stay as above.
 *  SampleEvents draws coordinate d of an event that picked row i from N(s_id, (h_d lambda_i)^2) truncated to the domain;
 *  the Philox words, counters, rounding and clamp rules are unchanged.  Project is, per sample and bin,
 *    [Phi((t_j+1 - u_i)/lambda_i) - Phi((t_j - u_i)/lambda_i)] / [Phi((T - u_i)/lambda_i) - Phi(-u_i/lambda_i)].
 *  Deterministic: no floating-point atomics; the pilot's split over workgroups depends on the sample count alone and
 *  the splits are added in order, so two constructions, on any device, give the same lambda bits (per-device
 *  evaluators of a multi-GPU ensemble agree).  Share() and the SharedSamples constructor carry the sensitivity and the
 *  factors over; they are not recomputed.
 *  Accuracy: tests/kde_adaptive_reference.py has the bound; against the fixed-bandwidth bound the coordinate term
 *  grows with the 1/lambda_i^2 of the samples in reach of the point, at most 100 by the clips.
 *  Cost: one more multiply per pair and rows of D + 2 floats; the pilot is O(samples^2) in f64, once.
 *
 *  Cross-validated bandwidth scales (Silverman 3.4.4): CrossValidated(...) instead of the constructor, or
 *  SelectBandwidthScale / CvScores on an evaluator.  All in f64 on the f64 values of the float table at zero
 *  systematics, over the m untransformed rows inside the domain (with max_rows > 0 and n > max_rows every
 *  ceil(n / max_rows)-th of them in table order; m < 2 throws):
 *    M_jd(h)  = Phi((U_d - x_jd)/h_d) - Phi((L_d - x_jd)/h_d)            (Phi through erfc, as the prepass and the pilot)
 *    f_-i(h)  = 1/(m-1) sum_{j != i} prod_d phi((x_id - x_jd)/h_d) / (h_d M_jd(h))
 *    score(h) = (1/m) sum_i ln f_-i(h)
 *  The pair j == i is left out of the sum, never subtracted afterwards; a row with f_-i = 0 contributes -inf, the
 *  candidate then scores -inf and is never chosen.  Candidates of a search are h_cd = s_c sigma_d m^(-1/(D+4)), sigma_d
 *  this evaluator's own standard deviation over all n in-domain rows: n^(-1/(D+4)) is the exponent Scott's rule and the
 *  AMISE optimum share, so a multiplier found on m rows carries over to n.  Multipliers s_k = lo (hi/lo)^(k/(steps-1))
 *  (default 1/8 .. 4 in 21 steps: ratio 2^(1/4), 1 on the grid; at most 32 steps).  The largest finite score wins; a
 *  tie goes to the smaller |ln s|, then the smaller s; no finite score throws.  The search is one scan of a common
 *  multiplier on all observables, then (per_observable) one coordinate scan per observable in order with the others
 *  held at the values chosen so far, so the chosen score never decreases.  It chooses the GLOBAL scales, the Scott
 *  stage: with a sensitivity > 0 the pilot and the factors are then taken at the chosen bandwidths, exactly as if the
 *  scales had been typed in.  Deterministic: no floating-point atomics, the split over workgroups depends on m and the
 *  candidate count alone, partial sums are added in split order and the m logarithms on the host in table order -- two
 *  calls, a Share()d evaluator and any device give the same score bits.  An evaluator's own bandwidths never change.
 *  Accuracy: the bound of tests/kde_cv_reference.py.  Cost O(m^2 K) per scan of K candidates.
 *
 *  Cutoff radius: SetCutoff(R), R in units of each sample's own bandwidth (h_d, or h_d lambda_i when adaptive).  Opt-in,
 *  and an approximation whose error is the bound stated here.  R = 0, the default, is everything above: the same
 *  kernels, the same row layout, the same bits.  Accepted: 0, or 1 <= R <= +infinity; anything else, NaN included, throws.
 *    qcut   = R^2 log2(e) / 2, as an f32 rounded up.
 *    q'     of a pair = g_i sum_d (c_pd - c_id)^2 exactly as the pair kernels compute it in f32, c the coordinates
 *             scaled by sqrt(log2(e) / 2) / h_d and g_i = 1 / lambda_i^2 (1 for fixed bandwidths).
 *    A pair is dropped only if the kernel's own f32 q' for it would have been >= qcut; pairs below qcut are always
 *    summed.  A value therefore lies between the full sum and the sum over the pairs with q' < qcut, and each dropped
 *    term is at most W_i 2^-qcut.  The PDF no longer integrates to exactly 1: it falls short by at most the dropped
 *    mass.  From R = 15 (qcut > 149) every dropped exp2 is exactly 0 in f32 and the values are those of R = +infinity
 *    bit for bit; R = +infinity drops nothing but sums in the sorted order below.
 *  Pairs are dropped a 256-sample tile at a time, against a wave of 64 points at a time.  When a cutoff is first set the
 *  host orders the table rows by their untransformed coordinates clamped to the domain (a plain sort for one observable,
 *  else the Morton order of a fixed cell grid over [lower, upper); stable, ties by table index), once per table; it is
 *  kept on the device and Share()d evaluators use it and copy R.  Per evaluation, after the unchanged prepass, one more
 *  launch copies the rows into that order and writes each tile's box from the MOVED samples (min and max of c_d over
 *  the rows with weight > 0, their smallest g when adaptive), which makes the culling exact under any systematic; a tile
 *  without such a row is never visited.  SetEvalPoints sorts the live points by the same key, the others last, with one
 *  box per wave over live points only; values still go to pdf_out[offset + stride * i] for the caller's i.  Per wave and
 *  tile gap_d = max(0, tile_lo_d - wave_hi_d, wave_lo_d - tile_hi_d), and q_lb from the gaps by the pair's own operation
 *  sequence times the tile's smallest g; rounding is monotone, so every pair of that wave and tile has q' >= q_lb with
 *  no margin, and the tile is visited iff q_lb < qcut (sxmc_amd/csrc/kde_cutoff.h).  f32 within a visited tile, f64
 *  across the visited tiles in tile order.
 *  What does not change: the norm, the point codes, the NaN and 0 rules, norm == 0; Bandwidths, LocalFactors,
 *  cross-validation and the pilot; SampleEvents and Project, which keep reading the prepass's rows in table order and
 *  return the bytes of the same evaluator at R = 0.  What does: a point's value depends on which other points share its
 *  wave, always inside the envelope above.  Two evaluations, a shared evaluator and any device still give the same bits:
 *  no floating-point atomics, and the tiles a wave visits depend on the data alone.  EvalOnStream stays capture-safe:
 *  every buffer is allocated by SetCutoff or SetEvalPoints.  SetCutoff needs an idle evaluator and throws while a graph
 *  is being recorded; it plans the points again if they are already set.  Accuracy: tests/kde_cutoff_reference.py. */
class EvalKernel : public detail::EvalOver<detail::KernelApi> {
 public:
  typedef KernelCvOptions CvOptions;
  typedef KernelCvScan CvScan;
  typedef KernelCvResult CvResult;

  /** Bandwidth scales by leave-one-out likelihood cross-validation (Silverman 3.4.4; the contract is written out at
   *  sxmc_kde_cv_scores in include/sxmc_hip.h): over the m untransformed in-domain rows (every ceil(n / max_rows)-th
   *  when n > max_rows), in f64,
   *      M_jd(h) = Phi((U_d - x_jd)/h_d) - Phi((L_d - x_jd)/h_d),
   *      f_-i(h) = 1/(m-1) sum_{j != i} prod_d phi((x_id - x_jd)/h_d) / (h_d M_jd(h)),   score(h) = (1/m) sum_i ln f_-i(h),
   *  the pair j == i left out of the sum (never subtracted), a row with f_-i = 0 making the score -inf, m < 2 an
   *  error; candidates h_cd = s_c sigma_d m^(-1/(D+4)) with sigma_d over all n rows, so that a multiplier found on m
   *  rows carries over to n; the largest finite score wins, a tie going to the smaller |ln s|, then the smaller s.
   *  A provisional fixed-bandwidth evaluator at scale 1 runs the search; the evaluator returned is constructed with
   *  the chosen scales and the asked sensitivity, exactly as if the scales had been typed in (an adaptive evaluator's
   *  pilot and factors are taken at the chosen bandwidths).  No floating-point atomics; the same bits on any device.
   *  The caller deletes the evaluator. */
  static EvalKernel* CrossValidated(const std::vector<float>& samples, int nfields, int nobservables,
                                    const std::vector<double>& lower, const std::vector<double>& upper,
                                    const CvOptions& options = CvOptions(), unsigned dataset = 0,
                                    double bandwidth_sensitivity = 0.0) {
    CvResult report;
    {
      const EvalKernel pilot(samples, nfields, nobservables, lower, upper,
                             std::vector<double>((size_t)(nobservables > 0 ? nobservables : 0), 1.0), dataset);
      report = pilot.SelectBandwidthScale(options);
    }
    EvalKernel* k = new EvalKernel(samples, nfields, nobservables, lower, upper, report.scale, dataset,
                                   bandwidth_sensitivity);
    k->cv_report = report;
    k->cross_validated = true;
    return k;
  }

  /** score(h) of each absolute candidate bandwidth vector (candidates[c * nobservables + d], at most 32 of them) on
   *  this evaluator's table; no search.  rows_used: m. */
  std::vector<double> CvScores(const std::vector<double>& candidates, size_t max_rows = 0,
                               size_t* rows_used = nullptr) const {
    if (nobservables <= 0 || candidates.size() % (size_t)nobservables != 0) {
      throw Error("Number of candidate bandwidths not divisible by number of observables.");
    }
    std::vector<double> scores(candidates.size() / (size_t)nobservables);
    double none = 0.0;
    throw_on(sxmc_kde_cv_scores(handle, candidates.data(), (int)scores.size(), max_rows,
                                scores.empty() ? &none : scores.data(), rows_used));
    return scores;
  }

  /** The search on this evaluator's table; its own bandwidths do not change. */
  CvResult SelectBandwidthScale(const CvOptions& o = CvOptions()) const {
    const size_t D = (size_t)nobservables, steps = (size_t)(o.steps > 0 ? o.steps : 1);
    CvResult r;
    r.scale.assign(D, 0.0);
    r.at_edge.assign(D, 0);
    std::vector<double> grid((1 + D) * steps, 0.0), scores((1 + D) * steps, 0.0);
    std::vector<int> chosen(1 + D, -1);
    int nscans = 0;
    throw_on(sxmc_kde_cv_select(handle, o.lo, o.hi, o.steps, o.per_observable ? 1 : 0, o.max_rows, r.scale.data(), D,
                                &r.score, &r.score_at_one, r.at_edge.data(), &r.rows_used, &nscans, grid.data(),
                                scores.data(), chosen.data()));
    for (size_t s = 0; s < (size_t)nscans; s++) {
      CvScan scan;
      scan.observable = (int)s - 1;
      scan.grid.assign(grid.begin() + (long)(s * steps), grid.begin() + (long)((s + 1) * steps));
      scan.scores.assign(scores.begin() + (long)(s * steps), scores.begin() + (long)((s + 1) * steps));
      scan.chosen = chosen[s];
      r.scans.push_back(scan);
    }
    return r;
  }

  /** The bandwidth scales this evaluator was constructed with: typed in, or chosen by CrossValidated. */
  std::vector<double> BandwidthScale() const {
    std::vector<double> s((size_t)nobservables);
    throw_on(sxmc_kde_bandwidth_scale(handle, s.data(), s.size()));
    return s;
  }

  /** Whether CrossValidated made this evaluator (or the one it shares its table with), and that search's report. */
  bool CrossValidatedScales() const { return cross_validated; }
  const CvResult& CvReport() const { return cv_report; }

  EvalKernel(const std::vector<float>& samples, int nfields, int nobservables, const std::vector<double>& lower,
             const std::vector<double>& upper, const std::vector<double>& bandwidth_scale, unsigned dataset = 0,
             double bandwidth_sensitivity = 0.0)
      : EvalOver(nfields, nobservables, dataset) {
    throw_on(sxmc_kde_create_adaptive(samples.data(), samples.size(), 0, nfields, nobservables, lower.data(),
                                      lower.size(), upper.data(), upper.size(), bandwidth_scale.data(),
                                      bandwidth_scale.size(), dataset, bandwidth_sensitivity, &handle));
  }
  /** WEIGHTED MONTE CARLO SAMPLES: the same with one integer multiplicity per table row (sxmc_sample_multiplicities'
   *  fixed-point weights; the laws are written out at sxmc_kde_create_weighted in include/sxmc_hip.h).  Given here and
   *  never set afterwards: the bandwidths (Kish's n_eff = (sum m)^2 / sum m^2 where n stood, moments weighted by m), the
   *  pilot and the padding are fixed at construction.  The norm is sum m_i over the in-domain rows (a weighted
   *  EvalHist's, bit for bit); a row's weight is m_i / mass_i, so the pair sum, its cutoff and the combine are the code
   *  they were; SampleEvents picks a row with probability m_i / norm; Project weighs a row by m_i.  A count that is not
   *  the row count, or a total beyond 2^32 - 1, throws.  All m equal to a power of two give the unweighted evaluator's
   *  bytes.  An empty vector is NOT "no multiplicities": it is a count mismatch unless the table is empty.
   *  Cross-validation of such an evaluator (CvScores, SelectBandwidthScale) throws: not built.  Share() shares the column. */
  EvalKernel(const std::vector<float>& samples, int nfields, int nobservables, const std::vector<double>& lower,
             const std::vector<double>& upper, const std::vector<double>& bandwidth_scale,
             const std::vector<unsigned>& multiplicities, unsigned dataset = 0, double bandwidth_sensitivity = 0.0)
      : EvalOver(nfields, nobservables, dataset) {
    const unsigned none = 0;
    throw_on(sxmc_kde_create_weighted(samples.data(), samples.size(), 0, nfields, nobservables, lower.data(),
                                      lower.size(), upper.data(), upper.size(), bandwidth_scale.data(),
                                      bandwidth_scale.size(), dataset, bandwidth_sensitivity,
                                      multiplicities.empty() ? &none : multiplicities.data(), multiplicities.size(),
                                      &handle));
  }
  EvalKernel(const EvalKernel& base, SharedSamples s)
      : EvalOver(base, s), cv_report(base.cv_report), cross_validated(base.cross_validated) {}
  Eval* Share() const override { return new EvalKernel(*this, SharedSamples{}); }

  /** The multiplicities' total, or the row count when none are set: what n_mc is for either kind. */
  unsigned long long SampleTotal() const {
    unsigned long long total = 0;
    throw_on(sxmc_kde_sample_total(handle, &total));
    return total;
  }
  bool HasSampleMultiplicities() const {
    int is_set = 0;
    throw_on(sxmc_kde_get_sample_multiplicities(handle, nullptr, 0, &is_set));
    return is_set != 0;
  }
  /** The multiplicities; all 1 when none are set. */
  std::vector<unsigned> SampleMultiplicities() const {
    size_t n = 0;
    throw_on(sxmc_kde_nsamples(handle, &n));
    std::vector<unsigned> out(n);
    unsigned none = 0;
    throw_on(sxmc_kde_get_sample_multiplicities(handle, n ? out.data() : &none, n, nullptr));
    return out;
  }
  /** Kish's n_eff of the bandwidth rule; the in-domain row count when no multiplicities are set. */
  double EffectiveSamples() const {
    double n_eff = 0.0;
    throw_on(sxmc_kde_effective_samples(handle, &n_eff));
    return n_eff;
  }

  /** The alpha this evaluator was constructed with (a shared evaluator: its base's). */
  double BandwidthSensitivity() const {
    double a = 0.0;
    throw_on(sxmc_kde_sensitivity(handle, &a));
    return a;
  }

  /** lambda_i of every table row, fixed at construction; all 1.0 at sensitivity 0. */
  std::vector<double> LocalFactors() const {
    size_t n = 0;
    throw_on(sxmc_kde_nsamples(handle, &n));
    std::vector<double> lambda(n);
    double none = 0.0;
    throw_on(sxmc_kde_local_factors(handle, n ? lambda.data() : &none, n));
    return lambda;
  }

  /** sxmc_kde_eval_on_stream_async: the launches of EvalAsync on the caller's stream (bindings made current first, as
   *  EvalAsync does), capture-safe; the evaluator orders its other calls after it.  For a walk that keeps its whole
   *  step on one stream. */
  void EvalOnStream(sxmc_stream_t stream, bool do_eval_pdf = true) {
    Bind();
    throw_on(sxmc_kde_eval_on_stream_async(handle, do_eval_pdf ? 1 : 0, stream));
  }

  /** The parameter indices the attached systematics read, before the parameter buffer's offset. */
  std::vector<short> ParametersRead() const {
    size_t n = 0;
    short none = 0;
    throw_on(sxmc_kde_parameters_read(handle, &none, 0, &n));
    std::vector<short> pars(n);
    if (n) throw_on(sxmc_kde_parameters_read(handle, pars.data(), n, &n));
    return pars;
  }

  /** Evaluations launched so far, by EvalAsync or EvalOnStream (a recorded launch counts once, when recorded). */
  unsigned long long EvaluationCount() const {
    unsigned long long n = 0;
    throw_on(sxmc_kde_evaluation_count(handle, &n));
    return n;
  }

  /** The cutoff radius (class comment, "Cutoff radius"; sxmc_kde_set_cutoff): 0 off, or 1 <= R <= +infinity. */
  void SetCutoff(double R) { throw_on(sxmc_kde_set_cutoff(handle, R)); }
  double Cutoff() const {
    double R = 0.0;
    throw_on(sxmc_kde_cutoff(handle, &R));
    return R;
  }
  /** Of the last evaluation: the tiles its waves visited, and live point-waves x tiles; both 0 without a cutoff. */
  void CutoffStats(unsigned long long& tiles_visited, unsigned long long& tiles_possible) const {
    throw_on(sxmc_kde_cutoff_stats(handle, &tiles_visited, &tiles_possible));
  }
  /** Of the current point plan: the pair sum's workgroups to every 256 points, and the sample tiles each walks. */
  void PairSplit(int& nsplit, unsigned& tiles_per_split) const {
    throw_on(sxmc_kde_pair_split(handle, &nsplit, &tiles_per_split));
  }

  /** The bandwidths h_d fixed at construction (Scott's rule). */
  std::vector<double> Bandwidths() const {
    std::vector<double> h((size_t)nobservables);
    throw_on(sxmc_kde_bandwidths(handle, h.data(), h.size()));
    return h;
  }

  /** sxmc_kde_project: per bin the analytic integral of every in-domain sample's truncated Gaussian, in f64; two
   *  calls give the same bits. */
  std::vector<double> Project(int obs, int nbins) override {
    std::vector<double> out((size_t)(nbins > 0 ? nbins : 0), 0.0);
    double none = 0.0;
    throw_on(sxmc_kde_project(handle, obs, nbins, out.empty() ? &none : out.data()));
    return out;
  }

 private:
  CvResult cv_report;
  bool cross_validated = false;
};

}  // namespace pdfz
