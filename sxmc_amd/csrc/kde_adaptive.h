// kde_adaptive.h -- the host arithmetic of an adaptive pdfz::EvalKernel (sxmc_kde_create_adaptive): Abramson's
// sample-point factors from the pilot estimate.  Plain C++ in f64 with no device call, so that a stand-alone program
// can include it (tests/cpp/kde_adaptive_host.cpp).  The contract is written out in include/sxmc_hip.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace sxkde {

constexpr double kFactorMin = 0.1, kFactorMax = 10.0;   // the clips of lambda
constexpr int kPilotSplits = 16;                        // at most this many workgroups share the pilot's samples
constexpr unsigned kPilotGrain = 256;                   // ... in whole multiples of this many samples

inline bool valid_sensitivity(double alpha) { return std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0; }

// How the pilot cuts its n in-domain samples over workgroups: from n alone, so every device adds the same partial sums
// in the same order.
inline void pilot_split(size_t n, unsigned& per_split, unsigned& nsplit) {
  const size_t share = (n + kPilotSplits - 1) / kPilotSplits;
  per_split = (unsigned)std::max<size_t>(kPilotGrain, (share + kPilotGrain - 1) / kPilotGrain * kPilotGrain);
  nsplit = (unsigned)std::max<size_t>(1, (n + per_split - 1) / per_split);
}

// g = exp(mean of ln f over the in-domain rows), added in table order.
inline double pilot_scale(const double* f, const std::vector<size_t>& inside) {
  double s = 0.0;
  for (size_t i : inside) s += std::log(f[i]);
  return std::exp(s / (double)inside.size());
}

// lambda = min(10, max(0.1, (f / g)^-alpha)); a pilot value that is not finite and positive takes 10.
inline double local_factor(double f, double g, double alpha) {
  if (!(std::isfinite(f) && f > 0.0)) return kFactorMax;
  const double l = std::pow(f / g, -alpha);
  if (!(l == l)) return kFactorMax;
  return std::min(kFactorMax, std::max(kFactorMin, l));
}

}  // namespace sxkde
