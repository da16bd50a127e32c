// sample_weights_walk.cpp -- walks of sxmc::MCMC over WEIGHTED MONTE CARLO SAMPLES (sample multiplicities,
// include/sxmc_hip.h), for tests/test_gpu_weighted_fill_walk.py.  The small fit's recipe (small_fit.h) at 3 000 + 333 j rows
// per signal, in four kinds: the tables as they are; every multiplicity 8 (n_mc = 8 n); multiplicities 0 ... 3 from the
// fit's own LCG; the tables with row i repeated m_i times.  Per form of the walk, 300 steps through both re-tunings:
//   times8 == plain and weighted == repeated, as the bytes of Chain::rows and the accepted steps.
// One line per form: "ok <form>" with the four hashes, or "FAIL <form>"; the exit status says whether all were ok.
// Without a GPU it says so and exits 0.
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

enum Kind { PLAIN, TIMES8, WEIGHTED, REPEATED };

struct Fit {
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> signals;
  std::vector<sxmc::Systematic> systematics;
  std::vector<sxmc::Observable> observables;
  std::vector<float> data;
  ~Fit() {
    for (sxmc::Signal& s : signals) delete s.histogram;
  }
  // with_kernel: a fourth, kernel-density signal (unweighted in every kind) beside the three histogram signals
  void build(Kind kind, int events_per_signal, bool with_kernel) {
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
    const int nsig = with_kernel ? 4 : 3;
    for (int j = 0; j < nsig; j++) {
      const bool kernel = j == 3;
      const size_t n = kernel ? 400 : 3000 + 333 * (size_t)j;
      std::vector<float> tab(n * 4), rep;
      std::vector<unsigned> mult(n);
      for (size_t i = 0; i < n; i++) {
        const float t = 0.2f + 0.2f * (float)j + 0.3f * SmallFit::uni(s);
        tab[i * 4 + 0] = t + 0.2f * (SmallFit::uni(s) - 0.5f);
        tab[i * 4 + 1] = 2.2f * SmallFit::uni(s) - 0.1f;
        tab[i * 4 + 2] = t;
        tab[i * 4 + 3] = 0;
        mult[i] = (SmallFit::lcg(s) >> 16) & 3u;
        for (unsigned r = 0; r < mult[i]; r++) rep.insert(rep.end(), tab.begin() + 4 * i, tab.begin() + 4 * i + 4);
      }
      sxmc::Signal sig;
      sig.name = "sig" + std::to_string(j);
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.0f, false);
      sig.nexpected = 100 + 50 * j;
      if (kernel) {
        sig.pdf = "kernel";
        sig.bandwidth_scale.assign(2, 1.0);
      } else if (kind == TIMES8) {
        sig.multiplicities.assign(n, 8u);
        sig.weight_log2_scale = 3;
      } else if (kind == WEIGHTED) {
        sig.multiplicities = mult;
      }
      sxmc::build_pdfz(sig, (kind == REPEATED && !kernel) ? rep : tab, 4, observables, systematics);
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
  size_t accepted, nrows;
  std::string form;
  std::vector<size_t> n_mc;
};

Walked walk(Kind kind, int events_per_signal, bool with_kernel, const std::function<void(sxmc::MCMC&)>& settings) {
  Fit fit;
  fit.build(kind, events_per_signal, with_kernel);
  sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
  m.optimize = false;
  settings(m);
  const sxmc::Chain c = m(fit.data, 300, 0.2f, false, 100);
  Walked w{fnv1a(c.rows.data(), c.rows.size() * 4), c.accepted, c.nrows(), m.WalkFormName(), {}};
  for (const sxmc::Signal& s : fit.signals) w.n_mc.push_back(s.n_mc);
  return w;
}

bool form(const std::string& name, int events_per_signal, bool with_kernel, const std::function<void(sxmc::MCMC&)>& settings) {
  const Walked plain = walk(PLAIN, events_per_signal, with_kernel, settings);
  const Walked times8 = walk(TIMES8, events_per_signal, with_kernel, settings);
  const Walked weighted = walk(WEIGHTED, events_per_signal, with_kernel, settings);
  const Walked repeated = walk(REPEATED, events_per_signal, with_kernel, settings);
  bool ok = plain.hash == times8.hash && plain.accepted == times8.accepted && weighted.hash == repeated.hash &&
            weighted.accepted == repeated.accepted && weighted.hash != plain.hash && plain.accepted > 0 &&
            plain.accepted < 300;
  for (size_t j = 0; j < 3; j++) ok = ok && times8.n_mc[j] == 8 * plain.n_mc[j] && weighted.n_mc[j] == repeated.n_mc[j];
  std::printf("%s %s\tplain %016llx times8 %016llx weighted %016llx repeated %016llx accepted %zu %zu %zu %zu forms %s %s\n",
              ok ? "ok" : "FAIL", name.c_str(), (unsigned long long)plain.hash, (unsigned long long)times8.hash,
              (unsigned long long)weighted.hash, (unsigned long long)repeated.hash, plain.accepted, times8.accepted,
              weighted.accepted, repeated.accepted, plain.form.c_str(), weighted.form.c_str());
  std::fflush(stdout);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  // sample_weights_walk two_launch: the consuming step with the cooperative step end switched off for the process (the
  // library reads SXMC_COOP_STEP_END once), i.e. ending in two launches; that form alone
  const bool two_launch = argc > 1 && std::string(argv[1]) == "two_launch";
  if (two_launch) setenv("SXMC_COOP_STEP_END", "0", 1);
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("sample_weights_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  bool ok = true;
  try {
    if (two_launch) return form("two_launch", 150, false, [](sxmc::MCMC&) {}) ? 0 : 1;
    ok = form("consuming", 150, false, [](sxmc::MCMC&) {}) && ok;
    ok = form("one_workgroup", 20, false, [](sxmc::MCMC&) {}) && ok;
    ok = form("reference_form", 150, false, [](sxmc::MCMC& m) { m.reference_form = true; }) && ok;
    ok = form("consume_off", 150, false, [](sxmc::MCMC& m) { m.consume = false; }) && ok;
    ok = form("graphs_of_16", 150, false, [](sxmc::MCMC& m) { m.graph_steps = 16; }) && ok;
    ok = form("lookahead_asked", 150, false, [](sxmc::MCMC& m) { m.lookahead = true; }) && ok;
    ok = form("mixed", 100, true, [](sxmc::MCMC&) {}) && ok;
    {
      // a lockstep set has no weighted fill: the walker says so by name
      Fit fit;
      fit.build(WEIGHTED, 150, false);
      sxmc::LockstepSet set(2, nullptr);
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      m.lockstep = &set;
      std::string said = "nothing";
      try {
        m(fit.data, 20, 0.2f, false, 100);
      } catch (const pdfz::Error& e) {
        said = e.msg;
      }
      const bool refused = said.find("a lockstep set has no weighted fill") != std::string::npos;
      std::printf("%s lockstep_refused\t%s\n", refused ? "ok" : "FAIL", said.c_str());
      ok = ok && refused;
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "sample_weights_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sample_weights_walk: %s\n", e.what());
    return 1;
  }
  return ok ? 0 : 1;
}
