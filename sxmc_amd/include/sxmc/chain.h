// chain.h -- the sampled likelihood space an MCMC walk returns (mcmc.h) and the interval extraction reads
// (intervals.h).  The standard library only.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

namespace sxmc {

/** The sampled likelihood space: one row per kept step = parameters..., likelihood (mcmc.cpp:100-114). */
struct Chain {
  std::vector<std::string> names;  //!< parameter names, then "likelihood"
  std::vector<float> rows;         //!< row-major [nrows][names.size()]
  size_t accepted = 0;             //!< accepted proposals over the whole walk
  double setup_seconds = 0;        //!< of the walk that made it: entry to the first step (buffers, SetEvalPoints, first
                                   //!< evaluation, launch-shape trials), host clock
  double steps_seconds = 0;        //!< ... and the steps themselves, re-tunings, flushes and graph recording included
  size_t nrows() const { return names.empty() ? 0 : rows.size() / names.size(); }
  float at(size_t row, size_t col) const { return rows[row * names.size() + col]; }
};

}  // namespace sxmc
