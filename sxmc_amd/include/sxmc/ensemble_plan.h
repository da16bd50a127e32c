// ensemble_plan.h -- how ensemble_multi_gpu (multi_gpu.h) shares N experiments of P parameters among G ranks and
// brings their intervals back, as pure functions: experiment k runs on rank k mod G as that rank's k / G-th; every
// rank contributes ONE block of ceil(N / G) slots of P x 4 floats (point estimate, lower, upper, coverage:
// interval.h:22-27), filled with NaN where it has no experiment; rank 0's copy of the G blocks, put back into
// experiment order, gives the medians.  No library call and no project header: the standard library only, so that
// tests/cpp/test_ensemble_plan.cpp checks every rule here without a device.  multi_gpu.h calls these and keeps no
// second copy of any of them.
#pragma once

#include <cstddef>
#include <limits>
#include <vector>

namespace sxmc {

struct ShardPlan {
  size_t G, N, P;   //!< ranks (> 0), experiments, parameters

  size_t per() const { return (N + G - 1) / G; }   //!< slots per rank
  size_t slot_floats() const { return P * 4; }
  size_t block() const { return per() * slot_floats(); }   //!< floats every rank sends
  size_t rank_of(size_t k) const { return k % G; }
  size_t slot_of(size_t k) const { return k / G; }
  /** Rank r's experiments, in the order of its slots: r, r + G, ... */
  std::vector<unsigned> experiments_of(size_t r) const {
    std::vector<unsigned> ks;
    for (size_t k = r; k < N; k += G) ks.push_back((unsigned)k);
    return ks;
  }
  /** Where floats are kept for `blocks` blocks, no slot filled yet. */
  std::vector<float> empty_blocks(size_t blocks = 1) const {
    return std::vector<float>(blocks * block(), std::numeric_limits<float>::quiet_NaN());
  }
  /** The intervals of a rank's i-th experiment into slot i of its block.  Iv: anything with the four float members
   *  named below (sxmc::Interval); parameters beyond P, or missing ones, are left out, respectively left NaN. */
  template <typename Iv>
  void pack(std::vector<float>& block_floats, size_t i, const std::vector<Iv>& intervals) const {
    for (size_t p = 0; p < P && p < intervals.size(); p++) {
      float* at = &block_floats[(i * P + p) * 4];
      at[0] = intervals[p].point_estimate;
      at[1] = intervals[p].lower;
      at[2] = intervals[p].upper;
      at[3] = intervals[p].coverage;
    }
  }
  /** The G blocks, rank after rank, as [N][P][4] in experiment order.  The padding slots are not copied. */
  std::vector<float> unpack(const std::vector<float>& blocks) const {
    std::vector<float> gathered(N * slot_floats(), 0.0f);
    for (size_t k = 0; k < N; k++) {
      const float* from = blocks.data() + rank_of(k) * block() + slot_of(k) * slot_floats();
      for (size_t j = 0; j < slot_floats(); j++) gathered[k * slot_floats() + j] = from[j];
    }
    return gathered;
  }
  /** Per parameter, `median` (utils.h:76-90: sxmc::median<float>, passed in to keep this file on its own) over the
   *  experiments of the upper limit in `gathered`; 0 without experiments. */
  template <typename Median>
  std::vector<float> median_upper(const std::vector<float>& gathered, Median median) const {
    std::vector<float> out;
    for (size_t p = 0; p < P; p++) {
      std::vector<float> ups;
      for (size_t k = 0; k < N; k++) ups.push_back(gathered[(k * P + p) * 4 + 2]);
      out.push_back(ups.empty() ? 0.0f : median(ups));
    }
    return out;
  }
};

}  // namespace sxmc
