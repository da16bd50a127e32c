// kde_adaptive_host.cpp -- the host arithmetic of the adaptive kernel-density evaluator (sxmc_amd/csrc/kde_adaptive.h:
// the sensitivity's validation, the pilot's split, the scale g and the factors lambda) checked without a device or the
// library.  Stand-alone, so that tests/test_kde_adaptive_cpu.py can also build and run it under ASan + UBSan.
// Exit status 0 and "kde_adaptive_host: ok" when every check holds.
#include <cstdio>
#include <limits>

#include "../../sxmc_amd/csrc/kde_adaptive.h"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("kde_adaptive_host: line %d: %s\n", __LINE__, #cond);    \
      failures++;                                                          \
    }                                                                      \
  } while (0)

int main() {
  using namespace sxkde;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(valid_sensitivity(0.0) && valid_sensitivity(0.5) && valid_sensitivity(1.0));
  CHECK(!valid_sensitivity(-1e-9) && !valid_sensitivity(1.0000001) && !valid_sensitivity(nan) && !valid_sensitivity(inf));

  // the split: from n alone, whole grains, covers n, at most kPilotSplits workgroups
  for (size_t n : {size_t(2), size_t(255), size_t(256), size_t(257), size_t(3000), size_t(4096), size_t(4097),
                   size_t(131072), size_t(1000003)}) {
    unsigned per = 0, ns = 0;
    pilot_split(n, per, ns);
    CHECK(per % kPilotGrain == 0 && per >= kPilotGrain);
    CHECK(ns >= 1 && ns <= (unsigned)kPilotSplits);
    CHECK((size_t)ns * per >= n && (size_t)(ns - 1) * per < n);
  }
  unsigned per = 0, ns = 0;
  pilot_split(3000, per, ns);
  CHECK(per == 256 && ns == 12);

  // g is the geometric mean over the listed rows, in their order; the factors have geometric mean 1 when none clips
  const std::vector<double> f = {0.5, 2.0, 7.0, 1.0, 0.25, 4.0};
  const std::vector<size_t> inside = {0, 1, 3, 4, 5};   // row 2 is outside the domain
  const double g = pilot_scale(f.data(), inside);
  CHECK(std::fabs(g - 1.0) < 1e-15);
  for (double alpha : {0.25, 0.5, 1.0}) {
    double sum = 0.0;
    for (size_t i : inside) sum += std::log(local_factor(f[i], g, alpha));
    CHECK(std::fabs(sum) < 1e-14);
    CHECK(std::fabs(local_factor(4.0, g, alpha) - std::pow(4.0, -alpha)) < 1e-15);
  }
  CHECK(local_factor(1e6, 1.0, 1.0) == kFactorMin && local_factor(1e-6, 1.0, 1.0) == kFactorMax);
  CHECK(local_factor(0.0, 1.0, 0.5) == kFactorMax && local_factor(-1.0, 1.0, 0.5) == kFactorMax);
  CHECK(local_factor(nan, 1.0, 0.5) == kFactorMax && local_factor(inf, 1.0, 0.5) == kFactorMax);
  CHECK(local_factor(1e-320, 1e-300, 1.0) == kFactorMax);   // a subnormal pilot value is positive and finite: clipped
  if (failures == 0) std::printf("kde_adaptive_host: ok\n");
  return failures ? 1 : 0;
}
