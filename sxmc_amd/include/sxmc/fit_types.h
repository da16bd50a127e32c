// fit_types.h -- ROOT- and JSON-free forms of the reference's fit metadata structs, with the
// reference's field names, as far as the MCMC driver needs them:
//   Source      src/source.h:13-58        Observable  src/observable.h:22-42
//   Systematic  src/systematic.h:23-49    Signal      src/signal.h (name, dataset, source, nexpected,
//                                                       n_mc, histogram)
// Callers fill these structs directly, or sxmc::load_config (config.h: the reference's JSON schema, config.cpp:19-297,
// and ROOT-free sample tables in place of io/ttree_io.cpp) fills them from a fit configuration.
#pragma once

#include <cstddef>
#include <memory>
#include <string>
#include <vector>

#include "pdfz.h"

namespace sxmc {

struct Source {
  Source() {}
  Source(const std::string& _name, size_t _index, float _mean, float _sigma, bool _fixed)
      : name(_name), index(_index), mean(_mean), sigma(_sigma), fixed(_fixed) {}
  std::string name;
  size_t index = 0;    //!< Index in the list of sources
  float mean = 1.0f;   //!< Mean expectation (scaling, 1.0 is nominal)
  float sigma = 0.0f;  //!< Gaussian constraint (fractional)
  bool fixed = false;
};

struct Observable {
  std::string name;
  std::string field;
  size_t field_index = 0;  //!< Index in the sampled data for this field
  size_t bins = 0;
  float lower = 0;
  float upper = 0;
};

struct Systematic {
  std::string name;
  std::string title;
  std::string observable_field;  //!< Name of the field the systematic acts on (systematic.h)
  std::string truth_field;       //!< resolution_scale: name of the field holding the true value
  size_t observable_field_index = 0;
  size_t truth_field_index = 0;
  size_t npars = 1;            //!< Number of parameters in power series
  std::vector<double> means;   //!< Mean values (power series)
  std::vector<double> sigmas;  //!< Standard deviations
  std::vector<short> pidx;     //!< Global indices into the systematic block of the parameter vector
  pdfz::Systematic::Type type = pdfz::Systematic::SHIFT;
  bool fixed = false;
};

struct Signal {
  std::string name;
  std::string title;
  std::string filename;                       //!< where the samples came from (signal.h)
  std::vector<std::string> systematic_names;  //!< the systematics this signal lists in the configuration
  unsigned dataset = 0;
  Source source;
  double nexpected = 0;
  size_t n_mc = 0;  //!< number of MC samples BEFORE cuts (signal.cpp:28); build_pdfz fills it in when it is 0.  With
                    //!< multiplicities: their total BEFORE cuts (bins, norm and n_mc all carry the scale 2^k: it cancels)
  std::vector<unsigned> multiplicities;       //!< either pdf: one per row of the table given to build_pdfz (after cuts), or empty:
                                              //!< every row counts once (include/sxmc_hip.h, sxmc_sample_multiplicities)
  int weight_log2_scale = 0;                  //!< ... the k of their scale 2^k: a row's weight is m * 2^-k
  std::string pdf = "hist";                   //!< "hist": pdfz::EvalHist; "kernel": pdfz::EvalKernel (kernel density)
  std::vector<double> bandwidth_scale;        //!< "kernel": one per fit observable, in fit-observable order (empty: 1.0)
  double bandwidth_sensitivity = 0.0;         //!< "kernel": alpha of the adaptive bandwidths in [0, 1]; 0: fixed
  double bandwidth_cutoff = 0.0;              //!< "kernel": cutoff radius of the pair sum in bandwidths; 0: none
  bool bandwidth_cv = false;                  //!< "kernel": bandwidth_scale is still to be chosen by cross-validation
                                              //!< (build_pdfz chooses, writes bandwidth_scale and clears the flag)
  pdfz::EvalKernel::CvOptions cv;             //!< ... on this grid, with this search
  pdfz::Eval* histogram = nullptr;  //!< borrowed by the driver, as in the reference
  // keeps the parameter-index arrays alive (the reference leaks them, signal.cpp:139)
  std::vector<std::shared_ptr<pdfz::Array<short>>> par_arrays;
};

/** Signal::build_pdfz (signal.cpp:112-170): the evaluator of one signal with every systematic attached -- a
 *  pdfz::EvalHist, or a pdfz::EvalKernel when sig.pdf is "kernel" (bandwidth scales from sig.bandwidth_scale, or chosen by
 *  cross-validation when sig.bandwidth_cv is set; the sensitivity of its adaptive bandwidths from
 *  sig.bandwidth_sensitivity, the cutoff radius of its pair sum from sig.bandwidth_cutoff).
 *  `samples` is the row-major [n][nfields] table, observables first. */
inline void build_pdfz(Signal& sig, const std::vector<float>& samples, int nfields,
                       const std::vector<Observable>& observables, std::vector<Systematic>& systematics) {
  std::vector<double> lower(observables.size()), upper(observables.size());
  std::vector<int> nbins(observables.size());
  for (const Observable& o : observables) {
    lower.at(o.field_index) = o.lower;
    upper.at(o.field_index) = o.upper;
    nbins.at(o.field_index) = (int)o.bins;
  }
  pdfz::Eval* h = nullptr;
  if (sig.pdf == "kernel") {
    const size_t D = observables.size();
    if (!sig.bandwidth_scale.empty() && sig.bandwidth_scale.size() != D) {
      throw pdfz::Error("signal '" + sig.name + "': " + std::to_string(sig.bandwidth_scale.size()) +
                        " bandwidth scales for " + std::to_string(D) + " observables");
    }
    std::vector<double> scale(D, 1.0);
    for (size_t i = 0; i < D && !sig.bandwidth_scale.empty(); i++) scale.at(observables[i].field_index) = sig.bandwidth_scale[i];
    if (!sig.multiplicities.empty()) {
      // weighted Monte Carlo samples: the same row-count check as for histograms; the evaluator takes them at construction
      if (sig.multiplicities.size() != samples.size() / (size_t)nfields) {
        throw pdfz::Error("signal '" + sig.name + "': " + std::to_string(sig.multiplicities.size()) + " multiplicities for " +
                          std::to_string(samples.size() / (size_t)nfields) + " rows");
      }
      if (sig.bandwidth_cv) {
        throw pdfz::Error("signal '" + sig.name + "': \"bandwidth_scale\": \"cv\" with sample multiplicities: cross-validation "
                          "of a weighted kernel-density evaluator is not built (the weighted leave-one-out score)");
      }
      h = new pdfz::EvalKernel(samples, nfields, (int)D, lower, upper, scale, sig.multiplicities, sig.dataset,
                               sig.bandwidth_sensitivity);
    } else if (sig.bandwidth_cv) {
      // "bandwidth_scale": "cv": chosen once, here; from now on the signal carries the numbers, so that every later
      // evaluator of it (another device's, a shared one) is built with them typed in and nothing is searched again
      pdfz::EvalKernel* k = pdfz::EvalKernel::CrossValidated(samples, nfields, (int)D, lower, upper, sig.cv, sig.dataset,
                                                             sig.bandwidth_sensitivity);
      const std::vector<double> chosen = k->BandwidthScale();
      sig.bandwidth_scale.assign(D, 1.0);
      for (size_t i = 0; i < D; i++) sig.bandwidth_scale[i] = chosen.at(observables[i].field_index);
      sig.bandwidth_cv = false;
      h = k;
    } else {
      h = new pdfz::EvalKernel(samples, nfields, (int)D, lower, upper, scale, sig.dataset, sig.bandwidth_sensitivity);
    }
    if (sig.bandwidth_cutoff != 0.0) static_cast<pdfz::EvalKernel*>(h)->SetCutoff(sig.bandwidth_cutoff);
  } else if (sig.pdf == "hist") {
    pdfz::EvalHist* hist = new pdfz::EvalHist(samples, nfields, (int)observables.size(), lower, upper, nbins, sig.dataset);
    h = hist;
    if (!sig.multiplicities.empty()) {
      if (sig.multiplicities.size() != samples.size() / (size_t)nfields) {
        delete hist;
        throw pdfz::Error("signal '" + sig.name + "': " + std::to_string(sig.multiplicities.size()) + " multiplicities for " +
                          std::to_string(samples.size() / (size_t)nfields) + " rows");
      }
      hist->SetSampleMultiplicities(sig.multiplicities);
    }
  } else {
    throw pdfz::Error("signal '" + sig.name + "': unknown pdf \"" + sig.pdf + "\" (\"hist\" or \"kernel\")");
  }
  sig.histogram = h;
  // (a table loaded through load_config has been cut: n_mc is then the row count before the cuts, set by the loader)
  if (sig.n_mc == 0) {
    sig.n_mc = samples.size() / (size_t)nfields;
    if (!sig.multiplicities.empty()) {
      sig.n_mc = sig.pdf == "kernel" ? (size_t)static_cast<pdfz::EvalKernel*>(h)->SampleTotal()
                                     : (size_t)static_cast<pdfz::EvalHist*>(h)->SampleTotal();
    }
  }
  for (Systematic& s : systematics) {
    auto pars = std::make_shared<pdfz::Array<short>>(s.npars, true);
    for (size_t i = 0; i < s.pidx.size(); i++) pars->writeOnlyHostPtr()[i] = s.pidx[i];
    sig.par_arrays.push_back(pars);
    const int o = (int)s.observable_field_index, t = (int)s.truth_field_index;
    switch (s.type) {
      case pdfz::Systematic::SHIFT: h->AddSystematic(pdfz::ShiftSystematic(o, pars.get())); break;
      case pdfz::Systematic::SCALE: h->AddSystematic(pdfz::ScaleSystematic(o, pars.get())); break;
      case pdfz::Systematic::CTSCALE: h->AddSystematic(pdfz::CosThetaScaleSystematic(o, pars.get())); break;
      case pdfz::Systematic::RESOLUTION_SCALE:
        h->AddSystematic(pdfz::ResolutionScaleSystematic(o, t, pars.get()));
        break;
    }
  }
}

/** The signal's evaluator as the histogram evaluator it must be for `what`; a signal with another kind of evaluator (a
 *  pdfz::EvalKernel) throws a pdfz::Error that names it instead of dereferencing a failed cast. */
inline pdfz::EvalHist& histogram_of(const Signal& s, const std::string& what) {
  pdfz::EvalHist* h = dynamic_cast<pdfz::EvalHist*>(s.histogram);
  if (!h) throw pdfz::Error("signal '" + s.name + "': cannot " + what + ": its evaluator is not a pdfz::EvalHist");
  return *h;
}

/** A copy of `base` whose evaluator shares base's sample table (pdfz::Eval::Share): what each
 *  additional concurrent chain on a GPU works with.  The caller deletes .histogram, as for build_pdfz. */
inline Signal share_pdfz(const Signal& base) {
  Signal s = base;
  s.histogram = base.histogram->Share();
  return s;
}

/** Signal::get_efficiency (signal.cpp:172-199): fraction of the MC samples inside the PDF domain with
 *  every systematic at its mean. */
inline double get_efficiency(Signal& sig, const std::vector<Systematic>& systematics) {
  size_t npars = 0;
  for (const Systematic& s : systematics) npars += s.npars;
  pdfz::Array<double> param_buffer(npars, true);
  size_t k = 0;
  for (const Systematic& s : systematics)
    for (size_t j = 0; j < s.npars; j++) param_buffer.writeOnlyHostPtr()[k++] = s.means[j];
  pdfz::Array<unsigned> norms_buffer(1, true);
  norms_buffer.writeOnlyHostPtr();
  sig.histogram->SetNormalizationBuffer(&norms_buffer);
  sig.histogram->SetParameterBuffer(&param_buffer);
  sig.histogram->EvalAsync(false);
  sig.histogram->EvalFinished();
  const double in_domain = norms_buffer.readOnlyHostPtr()[0];
  sig.histogram->ForgetBuffers();   // the two arrays above die with this call
  return 1.0 * in_domain / (double)sig.n_mc;
}

}  // namespace sxmc
