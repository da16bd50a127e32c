// kde_plan.h -- the pure parts of pdfz::EvalKernel's evaluation plan: how the pair sum and the projection are split over
// workgroups, which rows of the untransformed table lie inside the domain, and the truncation mass of one Gaussian.
// Plain C++ with no device call, so that a stand-alone program can include it (tests/cpp/test_kde_plan.cpp); the mass is
// one inline host/device function, which the prepass and the cross-validation weights (kde_kernels.hip) and the
// pilot's set-up on the host (sxmc_kde.cpp) all run: the same operations in the same order, so the same bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#ifndef SXKDE_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SXKDE_HD __host__ __device__
#else
#define SXKDE_HD
#endif
#endif

namespace sxkde {

constexpr unsigned long long kPlanTile = 256;        // SXMC_KDE_TILE
constexpr unsigned long long kPlanProjLanes = 64;    // SXMC_KDE_PROJ_LANES
constexpr unsigned long long kPlanProjSplits = 1024;

// How the pair sum is split over workgroups: s splits of the sample tiles, each a workgroup per 256 points.  Of the
// splits that keep every workgroup's share whole, the one with the fewest rounds of `slots` resident workgroups times
// tiles per workgroup (the smallest on a tie).
inline void pair_split(size_t pitch, size_t ntiles, int cus, int& nsplit, unsigned& tiles_per_split) {
  const unsigned long long pblocks = pitch / 256, slots = (unsigned long long)cus * 8;
  unsigned long long best = ~0ull;
  nsplit = 1;
  tiles_per_split = (unsigned)ntiles;
  const unsigned long long smax = std::min<unsigned long long>(ntiles, std::max<unsigned long long>(1, 64 * slots / pblocks));
  for (unsigned long long s = 1; s <= smax; s++) {
    const unsigned long long tps = (ntiles + s - 1) / s;
    const unsigned long long used = (ntiles + tps - 1) / tps;
    const unsigned long long cost = (pblocks * used + slots - 1) / slots * tps;
    if (cost < best) {
      best = cost;
      nsplit = (int)used;
      tiles_per_split = (unsigned)tps;
    }
  }
}

// The projection's split: the npad sample rows are cut the same way on every device, into at most 1024 splits of whole
// tiles; the bins are rounded up to whole waves of lanes.
inline void project_split(unsigned long long npad, unsigned long long nbins, unsigned& rows_per_split, unsigned& nsplit,
                          unsigned long long& pitch) {
  rows_per_split = (unsigned)(((npad + kPlanProjSplits - 1) / kPlanProjSplits + kPlanTile - 1) / kPlanTile * kPlanTile);
  nsplit = (unsigned)((npad + rows_per_split - 1) / rows_per_split);
  pitch = (nbins + kPlanProjLanes - 1) / kPlanProjLanes * kPlanProjLanes;
}

// The rows of a table of n rows that lie inside the domain, in table order: observable d of row i stands at
// x[i * row_stride + d * col_stride] (row-major: (nfields, 1); column-major: (1, n)).  pdfz.cpp:388-398:
// lower <= x < upper in f64, written so that NaN fails.
inline std::vector<size_t> rows_inside(const float* x, size_t row_stride, size_t col_stride, size_t n, int D,
                                       const double* lower, const double* upper) {
  std::vector<size_t> inside;
  for (size_t i = 0; i < n; i++) {
    bool in = true;
    for (int d = 0; d < D; d++) {
      const double v = x[i * row_stride + (size_t)d * col_stride];
      in = in && v >= lower[d] && v < upper[d];
    }
    if (in) inside.push_back(i);
  }
  return inside;
}

// The mass of a Gaussian around x with bandwidth h inside [lower, upper), Phi((upper - x) / h) - Phi((lower - x) / h),
// with Phi(z) = erfc(-z / sqrt 2) / 2 and r = 1 / (h sqrt 2).
SXKDE_HD inline double truncation_mass(double x, double lower, double upper, double r) {
  return 0.5 * (erfc((x - upper) * r) - erfc((x - lower) * r));
}

}  // namespace sxkde
