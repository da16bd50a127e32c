// kde_cv.h -- the host arithmetic of likelihood cross-validation for pdfz::EvalKernel (sxmc_kde_cv_scores,
// sxmc_kde_cv_select): the multiplier grid, how a scan is cut over workgroups, which rows a subset scores, which
// candidate wins and the search over scans.  Plain C++ in f64 with no device call, so that a stand-alone program can
// include it (tests/cpp/kde_cv_host.cpp).  The contract is written out in include/sxmc_hip.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <string>
#include <vector>

namespace sxkde {

constexpr int kCvMaxCandidates = 32;                   // K of one scan: that many f64 accumulators to a lane
constexpr int kCvSplits = 16;                          // at most this many workgroups share a scan's sample rows
constexpr unsigned kCvGrain = 256;                     // ... in whole multiples of this many rows
constexpr unsigned long long kCvPartials = 1ull << 22; // ... while splits * m * K partial sums stay within this many

struct CvOptions {
  double lo = 0.125, hi = 4.0;   // first and last multiplier of Scott's rule
  int steps = 21;                // grid values: ratio 2^(1/4) by default, 1 on the grid
  bool per_observable = true;    // after the common scan, one coordinate scan per observable
  size_t max_rows = 65536;       // score at most this many rows (0: all)
};

// What is wrong with a grid, or null.
inline const char* cv_grid_error(double lo, double hi, int steps) {
  if (!(steps >= 1 && steps <= kCvMaxCandidates)) return "Cross-validation steps must be between 1 and 32.";
  if (!(std::isfinite(lo) && std::isfinite(hi) && lo > 0.0 && lo <= hi)) {
    return "Cross-validation grid needs 0 < lo <= hi, both finite.";
  }
  return nullptr;
}

// s_k = lo (hi / lo)^(k / (steps - 1)), taken as 2^(log2 lo + ((log2 hi - log2 lo) k) / (steps - 1)) so that powers of
// two on the grid (1 on the default one) are met exactly; the two ends are lo and hi themselves.
inline std::vector<double> cv_grid(double lo, double hi, int steps) {
  std::vector<double> s((size_t)steps);
  const double l0 = std::log2(lo), l1 = std::log2(hi);
  for (int k = 0; k < steps; k++) {
    s[(size_t)k] = steps == 1 ? lo : std::pow(2.0, l0 + ((l1 - l0) * (double)k) / (double)(steps - 1));
  }
  s[0] = lo;
  if (steps > 1) s[(size_t)steps - 1] = hi;
  return s;
}

// How a scan of K candidates cuts its m sample rows over workgroups: from m and K alone, so every device adds the same
// partial sums in the same order.  As pilot_split, with the number of splits also held to kCvPartials partial sums.
inline void cv_split(size_t m, int K, unsigned& per_split, unsigned& nsplit) {
  const unsigned long long terms = (unsigned long long)std::max<size_t>(m, 1) * (unsigned long long)std::max(K, 1);
  const unsigned long long room = kCvPartials / terms;
  const size_t splits = (size_t)std::min<unsigned long long>(kCvSplits, std::max<unsigned long long>(1, room));
  const size_t share = (m + splits - 1) / splits;
  per_split = (unsigned)std::max<size_t>(kCvGrain, (share + kCvGrain - 1) / kCvGrain * kCvGrain);
  nsplit = (unsigned)std::max<size_t>(1, (m + per_split - 1) / per_split);
}

// Which of the n in-domain rows (numbered in table order) are scored: every ceil(n / max_rows)-th from the first;
// max_rows == 0 scores all.
inline size_t cv_stride(size_t n, size_t max_rows) {
  if (max_rows == 0 || n <= max_rows) return 1;
  return (n + max_rows - 1) / max_rows;
}
inline size_t cv_subset_size(size_t n, size_t max_rows) {
  const size_t stride = cv_stride(n, max_rows);
  return (n + stride - 1) / stride;
}
inline std::vector<size_t> cv_subset(size_t n, size_t max_rows) {
  const size_t stride = cv_stride(n, max_rows);
  std::vector<size_t> idx;
  for (size_t i = 0; i < n; i += stride) idx.push_back(i);
  return idx;
}

// The winner of one scan: the largest finite score; a tie goes to the multiplier with the smaller |ln s|, then to the
// smaller s.  -1 when no score is finite.
inline int cv_choose(const std::vector<double>& grid, const std::vector<double>& scores) {
  int best = -1;
  for (size_t c = 0; c < grid.size() && c < scores.size(); c++) {
    if (!std::isfinite(scores[c])) continue;
    if (best < 0) {
      best = (int)c;
      continue;
    }
    const double sb = scores[(size_t)best];
    if (scores[c] > sb) {
      best = (int)c;
    } else if (scores[c] == sb) {
      const double a = std::fabs(std::log(grid[c])), b = std::fabs(std::log(grid[(size_t)best]));
      if (a < b || (a == b && grid[c] < grid[(size_t)best])) best = (int)c;
    }
  }
  return best;
}

struct CvScan {
  int observable = -1;          // -1: the common multiplier on all observables
  std::vector<double> grid;     // the multipliers tried (of `observable`, the others held)
  std::vector<double> scores;
  int chosen = -1;              // index into grid
};

struct CvReport {
  std::vector<double> scale;    // [D] the chosen multipliers of Scott's rule: a bandwidth_scale
  double score = 0.0;           // the score of the choice
  bool has_one = false;         // 1 is on the grid ...
  double score_at_one = std::numeric_limits<double>::quiet_NaN();   // ... and this the common scan's score there
  std::vector<CvScan> scans;    // the common scan, then (per_observable) one per observable in order
  std::vector<int> at_edge;     // [D] the choice sits on the first or last grid value: widen the grid
  size_t rows_used = 0;         // m
};

// The search: (a) one scan of a common multiplier on all observables; (b) with per_observable one round of coordinate
// scans in observable order over the same grid, the others held at the values chosen so far.  The value held is on the
// grid, so the chosen score never decreases from scan to scan.  score(mult, K, scores): the scores of K candidates,
// mult[c * D + d] the multiplier of observable d under candidate c; non-zero return stops the search with that code.
// Returns 0, the scorer's code, or -1 with `error` set when a scan has no finite score.
template <class Scorer>
int cv_search(const CvOptions& o, int D, Scorer&& score, CvReport& rep, std::string& error) {
  const std::vector<double> grid = cv_grid(o.lo, o.hi, o.steps);
  const int K = (int)grid.size();
  rep = CvReport();
  rep.scale.assign((size_t)D, 1.0);
  rep.at_edge.assign((size_t)D, 0);
  std::vector<double> mult((size_t)K * (size_t)D);
  const int nscans = o.per_observable ? 1 + D : 1;
  for (int scan = 0; scan < nscans; scan++) {
    const int obs = scan - 1;
    for (int c = 0; c < K; c++) {
      for (int d = 0; d < D; d++) {
        mult[(size_t)c * D + d] = (obs < 0 || d == obs) ? grid[(size_t)c] : rep.scale[(size_t)d];
      }
    }
    CvScan s;
    s.observable = obs;
    s.grid = grid;
    s.scores.assign((size_t)K, 0.0);
    if (int rc = score(mult.data(), K, s.scores.data())) return rc;
    s.chosen = cv_choose(s.grid, s.scores);
    if (s.chosen < 0) {
      error = "Cross-validation found no finite score: every candidate leaves some row without a neighbour in reach "
              "(widen the grid upwards).";
      return -1;
    }
    const bool edge = s.chosen == 0 || s.chosen == K - 1;
    for (int d = 0; d < D; d++) {
      if (obs < 0 || d == obs) {
        rep.scale[(size_t)d] = grid[(size_t)s.chosen];
        rep.at_edge[(size_t)d] = edge ? 1 : 0;
      }
    }
    rep.score = s.scores[(size_t)s.chosen];
    if (obs < 0) {
      for (int c = 0; c < K; c++) {
        if (grid[(size_t)c] == 1.0) {
          rep.has_one = true;
          rep.score_at_one = s.scores[(size_t)c];
        }
      }
    }
    rep.scans.push_back(std::move(s));
  }
  return 0;
}

}  // namespace sxkde
