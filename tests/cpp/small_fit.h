// small_fit.h -- the small fit of the C++ walk tests (test_cpp_api.cpp) and of the pinned walks (walk_dump.cpp): 3 signals
// of 20 000 + 777 j samples, 2 observables + a truth field + the dataset column, a shift and a resolution systematic,
// 450 events.
// Everything comes from one LCG, so every program that includes this builds the same tables and the same events.
#pragma once

#include <sxmc/pdfz.h>

#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/ensemble.h"

struct SmallFit {
  static unsigned lcg(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return s;
  }
  static float uni(unsigned& s) { return (lcg(s) >> 8) * (1.0f / 16777216.0f); }

  // 3 signals, 2 observables + truth + dataset, shift + resolution systematics
  void SetUp() {
    unsigned s = 12345;
    observables.resize(2);
    observables[0].field_index = 0; observables[0].bins = 12; observables[0].lower = 0; observables[0].upper = 1;
    observables[1].field_index = 1; observables[1].bins = 9; observables[1].lower = 0; observables[1].upper = 2;
    systematics.resize(2);
    systematics[0].name = "shift"; systematics[0].type = pdfz::Systematic::SHIFT;
    systematics[0].observable_field_index = 1; systematics[0].means = {0.0}; systematics[0].sigmas = {0.05};
    systematics[0].pidx = {0};
    systematics[1].name = "res"; systematics[1].type = pdfz::Systematic::RESOLUTION_SCALE;
    systematics[1].observable_field_index = 0; systematics[1].truth_field_index = 2;
    systematics[1].means = {0.0}; systematics[1].sigmas = {0.1}; systematics[1].pidx = {1};
    for (int j = 0; j < 3; j++) {
      const size_t n = 20000 + 777 * j;
      std::vector<float> tab(n * 4);
      for (size_t i = 0; i < n; i++) {
        const float t = 0.2f + 0.25f * j + 0.3f * uni(s);
        tab[i * 4 + 0] = t + 0.2f * (uni(s) - 0.5f);
        tab[i * 4 + 1] = 2.2f * uni(s) - 0.1f;
        tab[i * 4 + 2] = t;
        tab[i * 4 + 3] = 0;
      }
      sxmc::Signal sig;
      sig.name = "sig" + std::to_string(j);
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.0f, false);
      sig.nexpected = 100 + 50 * j;
      sxmc::build_pdfz(sig, tab, 4, observables, systematics);
      signals.push_back(sig);
      tables.push_back(tab);
      sources.push_back(sig.source);
      for (int e = 0; e < 150; e++) {
        const size_t i = lcg(s) % n;
        data.push_back(tab[i * 4 + 0]);
        data.push_back(tab[i * 4 + 1]);
        data.push_back(0);
      }
    }
  }
  void TearDown() {
    for (sxmc::Signal& s : signals) delete s.histogram;
  }
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> signals;
  std::vector<sxmc::Systematic> systematics;
  std::vector<sxmc::Observable> observables;
  std::vector<float> data;
  std::vector<std::vector<float>> tables;   // host copies of the sample tables (replicas on other GPUs)
};
