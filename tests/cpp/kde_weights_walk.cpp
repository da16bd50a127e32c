// kde_weights_walk.cpp -- walks of sxmc::MCMC over a kernel-density signal with WEIGHTED MONTE CARLO SAMPLES
// (sxmc_kde_create_weighted, include/sxmc_hip.h), for tests/test_gpu_kde_weighted_walk.py.  A small mixed fit: one
// histogram signal of 3 000 rows and one kernel-density signal of 400 rows that floats both systematics (shift +
// resolution scale), 300 events, 300 steps through both re-tunings.  Two kinds: the kernel signal as it is, and with every
// multiplicity 8 (build_pdfz then sets n_mc = 8 n).  Per form of the walk -- the reference form, the MIXED defaults,
// graphs of 16 steps --
//   times8 == plain, as the bytes of Chain::rows and the accepted steps (norm and n_mc both carry the scale).
// One line per form: "ok <form>" with the two hashes, or "FAIL <form>"; then build_pdfz's refusals by name.  The exit
// status says whether all were ok.  Without a GPU it says so and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "small_fit.h"

namespace {

uint64_t fnv1a(const void* data, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

enum Kind { PLAIN, TIMES8, SHORT_COLUMN, WITH_CV };

struct Fit {
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> signals;
  std::vector<sxmc::Systematic> systematics;
  std::vector<sxmc::Observable> observables;
  std::vector<float> data;
  ~Fit() {
    for (sxmc::Signal& s : signals) delete s.histogram;
  }
  void build(Kind kind, int events_per_signal) {
    unsigned s = 4321;
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
    for (int j = 0; j < 2; j++) {
      const bool kernel = j == 1;
      const size_t n = kernel ? 400 : 3000;
      std::vector<float> tab(n * 4);
      for (size_t i = 0; i < n; i++) {
        const float t = 0.3f + 0.2f * (float)j + 0.3f * SmallFit::uni(s);
        tab[i * 4 + 0] = t + 0.2f * (SmallFit::uni(s) - 0.5f);
        tab[i * 4 + 1] = 2.2f * SmallFit::uni(s) - 0.1f;
        tab[i * 4 + 2] = t;
        tab[i * 4 + 3] = 0;
      }
      sxmc::Signal sig;
      sig.name = "sig" + std::to_string(j);
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.0f, false);
      sig.nexpected = 100 + 50 * j;
      if (kernel) {
        sig.pdf = "kernel";
        sig.bandwidth_scale.assign(2, 1.0);
        if (kind != PLAIN) {
          sig.multiplicities.assign(kind == SHORT_COLUMN ? n - 1 : n, 8u);
          sig.weight_log2_scale = 3;
        }
        sig.bandwidth_cv = kind == WITH_CV;
      }
      sxmc::build_pdfz(sig, tab, 4, observables, systematics);
      signals.push_back(sig);
      sources.push_back(sig.source);
      for (int e = 0; e < events_per_signal; e++) {
        const size_t i = SmallFit::lcg(s) % n;
        data.push_back(tab[i * 4 + 0]);
        data.push_back(tab[i * 4 + 1]);
        data.push_back(0);
      }
    }
  }
};

struct Walked {
  uint64_t hash;
  size_t accepted;
  std::string form;
  size_t n_mc_kernel;
  unsigned long long total;
};

Walked walk(Kind kind, const std::function<void(sxmc::MCMC&)>& settings) {
  Fit fit;
  fit.build(kind, 150);
  sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
  m.optimize = false;
  settings(m);
  const sxmc::Chain c = m(fit.data, 300, 0.2f, false, 100);
  pdfz::EvalKernel* k = static_cast<pdfz::EvalKernel*>(fit.signals[1].histogram);
  return Walked{fnv1a(c.rows.data(), c.rows.size() * 4), c.accepted, m.WalkFormName(), fit.signals[1].n_mc,
                k->SampleTotal()};
}

bool form(const std::string& name, const std::function<void(sxmc::MCMC&)>& settings) {
  const Walked plain = walk(PLAIN, settings), times8 = walk(TIMES8, settings);
  const bool ok = plain.hash == times8.hash && plain.accepted == times8.accepted && plain.accepted > 0 &&
                  plain.accepted < 300 && plain.n_mc_kernel == 400 && times8.n_mc_kernel == 3200 &&
                  times8.total == 3200 && plain.total == 400 && plain.form == times8.form;
  std::printf("%s %s\tplain %016llx times8 %016llx accepted %zu %zu forms %s %s\n", ok ? "ok" : "FAIL", name.c_str(),
              (unsigned long long)plain.hash, (unsigned long long)times8.hash, plain.accepted, times8.accepted,
              plain.form.c_str(), times8.form.c_str());
  std::fflush(stdout);
  return ok;
}

bool refused(const std::string& name, Kind kind, const std::string& words) {
  std::string said = "nothing";
  try {
    Fit fit;
    fit.build(kind, 10);
  } catch (const pdfz::Error& e) {
    said = e.msg;
  }
  const bool ok = said.find(words) != std::string::npos;
  std::printf("%s %s\t%s\n", ok ? "ok" : "FAIL", name.c_str(), said.c_str());
  return ok;
}

}  // namespace

int main() {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("kde_weights_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  bool ok = true;
  try {
    ok = form("reference_form", [](sxmc::MCMC& m) { m.reference_form = true; }) && ok;
    ok = form("mixed", [](sxmc::MCMC&) {}) && ok;
    ok = form("graphs_of_16", [](sxmc::MCMC& m) { m.graph_steps = 16; }) && ok;
    ok = refused("row_count_refused", SHORT_COLUMN, "399 multiplicities for 400 rows") && ok;
    ok = refused("cv_refused", WITH_CV, "cross-validation of a weighted kernel-density evaluator is not built") && ok;
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "kde_weights_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "kde_weights_walk: %s\n", e.what());
    return 1;
  }
  return ok ? 0 : 1;
}
