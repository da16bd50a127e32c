// kde_weights.h -- the host arithmetic of a pdfz::EvalKernel over weighted Monte Carlo samples (sxmc_kde_create_weighted,
// sxmc_kde_weighted_bandwidths): the bandwidths of a table whose rows carry integer multiplicities, and the pilot's scale
// g.  Plain C++ in f64 with no device call, so that a stand-alone program can include it
// (tests/cpp/kde_weights_host.cpp).  The law is written out in include/sxmc_hip.h and restated in
// tests/kde_weighted_reference.py, which this file is held to bit for bit: one rounding per operation (build with
// -ffp-contract=off), every sum sequential in table order.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace sxkde {

constexpr int kWeightsMaxDim = 4;

enum WeightedBandwidthStatus {
  kWeightsOk = 0,
  kWeightsTooFew = 1,      // fewer than 2 in-domain rows with m > 0
  kWeightsNoFreedom = 2,   // S1 - S2 / S1 is not positive
  kWeightsNoSpread = 3,    // sigma_d == 0 (observable `observable`)
};

struct WeightedBandwidths {
  int status = kWeightsOk;
  int observable = -1;
  size_t live = 0;   // in-domain rows with m > 0
  double s1 = 0, s2 = 0, n_eff = 0;
  double mean[kWeightsMaxDim] = {0}, sigma[kWeightsMaxDim] = {0}, h[kWeightsMaxDim] = {0};
};

// Over the rows `inside` (table order) of the row-major table `rows` (`stride` floats to a row, observables first); m:
// one multiplicity per TABLE row, or null: every row counts once -- and then the numbers are those of the unweighted
// rule, byte for byte (S1 = S2 = n, n_eff = n, the denominator n - 1, every product by 1.0 exact).
//   S1 = sum m, S2 = sum m^2 (exact integers, 128 bits, each converted to double once); n_eff = S1 * (S1 / S2);
//   mu_d = (sum (double)m x_d) / S1; V_d = sum (double)m (dx dx), dx = x_d - mu_d; sigma_d = sqrt(V_d / (S1 - S2 / S1));
//   h_d = scale_d sigma_d pow(n_eff, -1 / (D + 4)).
// A power-of-two rescaling of every m leaves every byte of mu, sigma, n_eff and h as it was.
inline WeightedBandwidths weighted_bandwidths(const float* rows, size_t stride, const std::vector<size_t>& inside, int D,
                                              const double* scale, const unsigned* m) {
  WeightedBandwidths r;
  unsigned __int128 t1 = 0, t2 = 0;
  for (size_t i : inside) {
    const unsigned long long mi = m ? m[i] : 1u;
    t1 += mi;
    t2 += (unsigned __int128)mi * mi;
    r.live += mi > 0 ? 1 : 0;
  }
  r.s1 = (double)t1;
  r.s2 = (double)t2;
  if (r.live < 2) {
    r.status = kWeightsTooFew;
    return r;
  }
  const double ratio = r.s1 / r.s2;
  r.n_eff = r.s1 * ratio;
  const double back = r.s2 / r.s1;
  const double freedom = r.s1 - back;
  if (!(freedom > 0.0)) {
    r.status = kWeightsNoFreedom;
    return r;
  }
  const double expo = -1.0 / (D + 4);
  for (int d = 0; d < D; d++) {
    double sum = 0.0, v = 0.0;
    for (size_t i : inside) {
      const double mi = m ? (double)m[i] : 1.0;
      const double term = mi * (double)rows[i * stride + (size_t)d];
      sum = sum + term;
    }
    const double mean = sum / r.s1;
    for (size_t i : inside) {
      const double mi = m ? (double)m[i] : 1.0;
      const double dx = (double)rows[i * stride + (size_t)d] - mean;
      const double sq = dx * dx;
      const double term = mi * sq;
      v = v + term;
    }
    const double sigma = std::sqrt(v / freedom);
    r.mean[d] = mean;
    r.sigma[d] = sigma;
    if (!(sigma > 0.0)) {
      r.status = kWeightsNoSpread;
      r.observable = d;
      return r;
    }
    const double spread = scale[d] * sigma;
    r.h[d] = spread * std::pow(r.n_eff, expo);
  }
  return r;
}

// g = exp((sum (double)m_i ln f_i) / S1) over the in-domain rows in table order; a row of multiplicity 0 adds nothing
// (and its f_i, which may be 0 far from every weighted row, is not read).  m null: every row counts once.
inline double weighted_pilot_scale(const double* f, const std::vector<size_t>& inside, const unsigned* m, double s1) {
  double s = 0.0;
  for (size_t i : inside) {
    if (m && m[i] == 0u) continue;
    const double mi = m ? (double)m[i] : 1.0;
    const double term = mi * std::log(f[i]);
    s = s + term;
  }
  return std::exp(s / s1);
}

}  // namespace sxkde
