// sample_multiplicities.h -- real Monte Carlo sample weights as integer multiplicities on a power-of-two scale
// (include/sxmc_hip.h, sxmc_sample_multiplicities): pure host arithmetic, no device, no library state.  The one
// implementation behind the C ABI entry, which both loaders of a configuration's "weight_field" call;
// tests/cpp/sample_weights_host.cpp runs it stand-alone under ASan + UBSan, tests/sample_weights_reference.py restates it.
//
// The law.  For a candidate k, m_i = (unsigned) nearbyint(ldexp(w_i, k)) in the default rounding mode (half to even).
// k is the LARGEST integer in [-32, 24] for which every m_i <= 2^32 - 1 and sum m_i <= max_total; total = sum m_i in
// 64 bits.  A weight that is negative or not finite is refused (-0.0 is 0); so is a max_total beyond 2^32 - 1 (0 means
// 2^32 - 1), a set of weights no k fits, and one whose total comes out 0 at the chosen k (no rows, or all weights 0).
#pragma once

#include <cmath>
#include <cstddef>

namespace sxweights {

constexpr unsigned long long kMaxTotal = 0xFFFFFFFFull;
constexpr int kMinLog2 = -32, kMaxLog2 = 24;

enum class Status { ok, bad_max_total, bad_weight, no_scale, zero_total };
struct Result {
  Status status = Status::ok;
  size_t row = 0;                 // bad_weight: the first such row
  int log2_scale = 0;
  unsigned long long total = 0;
};

// m at scale k; false as soon as an m_i exceeds 2^32 - 1 or the running total exceeds max_total (m is then partly written)
inline bool multiplicities_at(const double* w, size_t n, int k, unsigned long long max_total, unsigned* m,
                              unsigned long long& total) {
  total = 0;
  for (size_t i = 0; i < n; i++) {
    const double r = std::nearbyint(std::ldexp(w[i], k));
    if (r > 4294967295.0) return false;
    const unsigned mi = (unsigned)r;
    total += mi;
    if (total > max_total) return false;
    m[i] = mi;
  }
  return true;
}

inline Result sample_multiplicities(const double* w, size_t n, unsigned long long max_total, unsigned* m) {
  Result res;
  if (max_total == 0) max_total = kMaxTotal;
  if (max_total > kMaxTotal) {
    res.status = Status::bad_max_total;
    return res;
  }
  double wmax = 0.0;
  for (size_t i = 0; i < n; i++) {
    if (!(w[i] >= 0.0) || std::isinf(w[i])) {
      res.status = Status::bad_weight;
      res.row = i;
      return res;
    }
    if (w[i] > wmax) wmax = w[i];
  }
  // (the largest weight alone rules out every k with wmax * 2^k >= 2^32: the search starts below those)
  int k = kMaxLog2;
  if (wmax > 0.0) k = std::fmin((double)kMaxLog2, 31.0 - (double)std::ilogb(wmax));
  for (; k >= kMinLog2; k--) {
    unsigned long long total = 0;
    if (!multiplicities_at(w, n, k, max_total, m, total)) continue;
    res.log2_scale = k;
    res.total = total;
    res.status = total == 0 ? Status::zero_total : Status::ok;
    return res;
  }
  res.status = Status::no_scale;
  return res;
}

}  // namespace sxweights
