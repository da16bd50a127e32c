// fake_data.h -- an experiment's fake data set, without ROOT.
//
//   make_fake_dataset            src/generator.cpp:10-48
//   EvalHist::RandomSample       src/pdfz.cpp:817-922 (TH1::GetRandom / GetRandom2 / GetRandom3: pick a bin
//                                with probability proportional to its content, then uniform inside the bin)
//
// Parity with the reference is statistical only: it draws on ROOT's generators.  Deviates come from std::mt19937_64 here.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>
#include <random>
#include <vector>

#include "fit_types.h"

namespace sxmc {

/** The float step of the histogram samplers (sxmc_hip.h, sxmc_hist_random_sample): (float)xd, moved one float at a time
 *  (at most 4) towards bin idx while the evaluator's look-up of the float -- lower <= x < upper and
 *  (int)((x - lower) * scale), in double -- does not give idx; a bin that holds no float at all: the in-domain float
 *  nearest to xd. */
inline float sample_float(double xd, size_t idx, double lower, double upper, double scale) {
  auto side = [&](float xf) {
    const double x = (double)xf;
    if (!(x >= lower)) return -1;
    if (!(x < upper)) return 1;
    const long long j = (long long)((x - lower) * scale);
    return j < (long long)idx ? -1 : j > (long long)idx ? 1 : 0;
  };
  const float inf = std::numeric_limits<float>::infinity();
  float xf = (float)xd;
  for (int step = 0; step < 4; step++) {
    const int s = side(xf);
    if (s == 0) return xf;
    xf = std::nextafter(xf, s < 0 ? inf : -inf);
  }
  if (side(xf) == 0) return xf;
  xf = (float)xd;
  if (!((double)xf >= lower)) {
    xf = (float)lower;
    if ((double)xf < lower) xf = std::nextafter(xf, inf);
  }
  if (!((double)xf < upper)) {
    xf = (float)upper;
    while (!((double)xf < upper)) xf = std::nextafter(xf, -inf);
  }
  return xf;
}

/** RandomSample on a flat row-major histogram (1-3 D): a bin in proportion to its content, a point uniform inside it,
 *  rounded to a float that the evaluator looks up into that bin (the device sampler's contract; the deviates here
 *  are the host generator's). */
inline void random_sample(std::mt19937_64& rng, const std::vector<unsigned>& bins, const std::vector<Observable>& obs,
                          size_t nobserved, unsigned dataset, std::vector<float>& events) {
  const size_t D = obs.size();
  if (D > 3) throw pdfz::Error("Cannot EvalHist::CreateHistogram for dimensions greater than 3!");
  std::vector<double> cdf(bins.size());
  double total = 0;
  for (size_t i = 0; i < bins.size(); i++) cdf[i] = (total += bins[i]);
  if (total <= 0) return;
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  for (size_t e = 0; e < nobserved; e++) {
    size_t flat = std::upper_bound(cdf.begin(), cdf.end(), uni(rng) * total) - cdf.begin();
    flat = std::min(flat, bins.size() - 1);
    std::vector<size_t> idx(D);
    for (size_t k = D; k-- > 0;) {
      idx[k] = flat % obs[k].bins;
      flat /= obs[k].bins;
    }
    for (size_t k = 0; k < D; k++) {
      const double lower = (double)obs[k].lower, upper = (double)obs[k].upper;
      const double width = (upper - lower) / (double)obs[k].bins;
      const double scale = (int)obs[k].bins / (upper - lower);   // the look-up's (pdfz.cpp:366-368)
      events.push_back(sample_float(lower + ((double)idx[k] + uni(rng)) * width, idx[k], lower, upper, scale));
    }
    events.push_back((float)dataset);
  }
}

/** make_fake_dataset (generator.cpp:10-48).  observables must be in field order. */
inline std::vector<float> make_fake_dataset(std::mt19937_64& rng, std::vector<Signal>& signals,
                                            std::vector<Systematic>& systematics,
                                            std::vector<Observable>& observables, bool poisson,
                                            std::vector<unsigned>* observed_out = nullptr) {
  std::vector<float> events;
  for (Signal& s : signals) {
    const double eff = get_efficiency(s, systematics);
    const double nevents = s.nexpected * eff;
    size_t observed;
    if (poisson) {
      observed = nevents > 0 ? std::poisson_distribution<long long>(nevents)(rng) : 0;
    } else {
      observed = (size_t)std::floor(nevents + 0.5);
    }
    if (observables.size() > 3 && dynamic_cast<pdfz::EvalHist*>(s.histogram)) {
      throw pdfz::Error("Cannot EvalHist::CreateHistogram for dimensions greater than 3!");
    }
    if (eff <= 0) observed = 0;   // an empty histogram yields no events
    // drawn on the device from the evaluation get_efficiency just made (a histogram's bins, or a kernel-density PDF's
    // moved samples): it never leaves HBM
    if (observed) s.histogram->SampleEvents(events, observed, rng());
    if (observed_out) observed_out->push_back((unsigned)observed);
  }
  return events;
}

/** The ASIMOV data set of a fit: one data set in which every bin holds its EXPECTED, non-integer content, as weighted
 *  events (sxmc::MCMC's operator() with event weights; one fit of it gives the median sensitivity). */
struct AsimovDataset {
  std::vector<float> events;       //!< rows in make_fake_dataset's layout: the observables, then the dataset id
  std::vector<double> weights;     //!< one per row
  std::vector<double> nexpected;   //!< per signal: nexpected_j * eff_j, what its rows' weights sum to
};

/** Per histogram signal j, evaluated at the nominal parameters exactly as get_efficiency does: nexp_j = nexpected_j *
 *  eff_j, and for every non-empty bin b in flat index order (last observable fastest) one row at the bin's centre --
 *  rounded with sample_float so that SetEvalPoints looks it up into b -- of weight nexp_j * c_b / sum(c), in double, left
 *  to right.  observables must be in field order.  Same rule as sxmc_amd.ensemble.make_asimov_dataset.  Kernel-density
 *  signals have no Asimov rule here: refused by name. */
inline AsimovDataset make_asimov_dataset(std::vector<Signal>& signals, std::vector<Systematic>& systematics,
                                         std::vector<Observable>& observables) {
  AsimovDataset out;
  const size_t D = observables.size();
  if (D > 3) throw pdfz::Error("Cannot EvalHist::CreateHistogram for dimensions greater than 3!");
  for (size_t j = 0; j < signals.size(); j++) {
    Signal& s = signals[j];
    pdfz::EvalHist* h = dynamic_cast<pdfz::EvalHist*>(s.histogram);
    if (!h) {
      throw pdfz::Error("make_asimov_dataset: signal " + std::to_string(j) +
                        " is a kernel-density signal: the Asimov data set is built from histogram signals only");
    }
    const double eff = get_efficiency(s, systematics);
    const double ne = s.nexpected * eff;
    out.nexpected.push_back(ne);
    const std::vector<unsigned> bins = h->GetBins();
    unsigned long long sum = 0;
    for (unsigned c : bins) sum += c;
    const double total = (double)sum;
    for (size_t b = 0; b < bins.size(); b++) {
      if (!bins[b]) continue;
      size_t flat = b;
      std::vector<size_t> idx(D);
      for (size_t k = D; k-- > 0;) {
        idx[k] = flat % observables[k].bins;
        flat /= observables[k].bins;
      }
      for (size_t k = 0; k < D; k++) {
        const double lower = (double)observables[k].lower, upper = (double)observables[k].upper;
        const double width = (upper - lower) / (double)observables[k].bins;
        const double scale = (int)observables[k].bins / (upper - lower);   // the look-up's (pdfz.cpp:366-368)
        out.events.push_back(sample_float(lower + ((double)idx[k] + 0.5) * width, idx[k], lower, upper, scale));
      }
      out.events.push_back((float)h->Dataset());
      out.weights.push_back(ne * (double)bins[b] / total);
    }
  }
  return out;
}

}  // namespace sxmc
