// weighted_walk.cpp -- walks of sxmc::MCMC over the small fit (small_fit.h) with WEIGHTED data events, for
// tests/test_gpu_weighted_walk.py.  Integer weights m_i in {1, 2, 3, 7} (from the fit's own LCG) against the data set in
// which event i stands m_i times.  One line per case: its name, a tab, then for the unweighted walk, the weighted walk
// and the walk over the repeated events the chain's rows, accepted steps and a 64-bit FNV-1a hash of the bytes of
// Chain::rows, and the form the walk took.  Then the refusals, one line each with what the walker said.
//   weighted_walk [DIR]
// With DIR: also writes the fit, the weights, the walk's initial widths and the default form's weighted chain there as raw
// native-order files, so that the Python walker can walk the same fit from the same widths and be compared byte for byte:
// table0.f32 .. table2.f32 (rows of 4 floats), data.f32 (rows of 3), weights.f64, widths.f32 (P), chain.f32 (rows of P + 1).
// seed 7, 600 steps, burn-in fraction 0.2 (both re-tunings fall inside), sync_interval 150, optimize off (a pinned chain
// must not depend on the timing of trial launches).  Without a GPU it says so and exits 0.
//   weighted_walk --bench [nsteps]   steps per second unweighted against all-ones weights on the small fit's recipe with 13
//                       signals of 200 000 samples (P = 15, the stand-in shape of proposal_walk --bench): warmed (2 000
//                       steps of each), then alternating twice, graph_steps 100, the default (consuming) form; the time is
//                       the walk's own host clock around its steps.  Default 30 000 steps.  Then ONE fit of that shape's
//                       Asimov data set (sxmc::make_asimov_dataset), the same steps, timed the same way.
//   weighted_walk --mixed   the same comparison over a fit that MIXES a histogram signal with kernel-density signals
//                       (tests/cpp/proposal_mixed_walk.cpp's: one observable of 25 bins and a truth field; `spectrum`, a
//                       histogram over 100 000 samples with a scale and a resolution systematic; `line`, kernel density
//                       over 2 000 samples with the same two; `pedestal`, kernel density over 800, none; about 800 events;
//                       seed 99): the MIXED form with its columns step end, replayed from graphs of 16 steps, with the
//                       plain step end (consume off), with the covariance proposal, and the reference form.
//   weighted_walk --config FIT.json DIR   the fit of a configuration (sxmc::load_config) through sxmc::ensemble with the
//                       configuration's "asimov" as the runner's option: prints how many experiments ran, the seed of the
//                       first and what the runner reported; writes to DIR the chains (chain_<k>.f32, rows of P + 1), the
//                       walk's initial widths (widths.f32) and sxmc::make_asimov_dataset's own output for the fit
//                       (asimov_rows.f32, asimov_weights.f64, asimov_nexp.f64), for comparison with sxmc_amd.io.run_config
//                       and ensemble.make_asimov_dataset.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "small_fit.h"
#include "../../sxmc_amd/include/sxmc/config.h"

namespace {

uint64_t fnv1a(const void* data, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

template <typename T>
void write_file(const std::string& path, const std::vector<T>& v) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
  std::fclose(f);
}

// proposal_walk --bench's "p15": the small fit's recipe, 13 signals of 200 000 samples, 150 events of each
struct BenchFit {
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> signals;
  std::vector<sxmc::Systematic> systematics;
  std::vector<sxmc::Observable> observables;
  std::vector<float> data;
  ~BenchFit() {
    for (sxmc::Signal& s : signals) delete s.histogram;
  }
  void build() {
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
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
    for (int j = 0; j < 13; j++) {
      const size_t n = 200000;
      std::vector<float> tab(n * 4);
      for (size_t i = 0; i < n; i++) {
        const float t = 0.1f + 0.06f * (float)j + 0.3f * uni(rng);
        tab[i * 4 + 0] = t + 0.2f * (uni(rng) - 0.5f);
        tab[i * 4 + 1] = 2.2f * uni(rng) - 0.1f;
        tab[i * 4 + 2] = t;
        tab[i * 4 + 3] = 0;
      }
      sxmc::Signal sig;
      sig.name = "sig" + std::to_string(j);
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.0f, false);
      sig.nexpected = 150;
      sxmc::build_pdfz(sig, tab, 4, observables, systematics);
      signals.push_back(sig);
      sources.push_back(sig.source);
      for (int e = 0; e < 150; e++) {
        const size_t i = rng() % n;
        data.push_back(tab[i * 4 + 0]);
        data.push_back(tab[i * 4 + 1]);
        data.push_back(0);
      }
    }
  }
};

int run_bench(unsigned nsteps) {
  try {
    BenchFit fit;
    fit.build();
    const std::vector<double> ones(fit.data.size() / 3, 1.0);
    auto one = [&](const char* label, bool weighted, unsigned steps, int repeat) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 1, nullptr);
      m.optimize = false;
      m.graph_steps = 100;
      const sxmc::Chain c = weighted ? m(fit.data, ones, steps, 0.2f, false, 10000) : m(fit.data, steps, 0.2f, false, 10000);
      std::printf("%s %s\trepeat %d steps %u form %s steps_per_second %.1f seconds %.4f fnv1a %016llx\n", label,
                  weighted ? "unit weights" : "unweighted", repeat, steps, m.WalkFormName(),
                  (double)steps / c.steps_seconds, c.steps_seconds,
                  (unsigned long long)fnv1a(c.rows.data(), c.rows.size() * 4));
      std::fflush(stdout);
    };
    for (int w = 0; w < 2; w++) one("warm-up", w == 1, 2000, 0);
    for (int repeat = 1; repeat <= 2; repeat++)
      for (int w = 0; w < 2; w++) one("p15", w == 1, nsteps, repeat);
    {
      // one Asimov fit of the shape: the data set's construction and the walk, each on the host clock
      const auto t0 = std::chrono::steady_clock::now();
      sxmc::AsimovDataset a = sxmc::make_asimov_dataset(fit.signals, fit.systematics, fit.observables);
      const double build = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 1, nullptr);
      m.optimize = false;
      m.graph_steps = 100;
      const sxmc::Chain c = m(a.events, a.weights, nsteps, 0.2f, false, 10000);
      std::printf("p15 asimov\trows %zu steps %u form %s steps_per_second %.1f build_seconds %.4f setup_seconds %.4f "
                  "seconds %.4f accepted %zu\n", a.weights.size(), nsteps, m.WalkFormName(),
                  (double)nsteps / c.steps_seconds, build, c.setup_seconds, c.steps_seconds, c.accepted);
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

struct MixedFit {
  std::vector<sxmc::Observable> observables;
  std::vector<sxmc::Systematic> systematics, none;
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> base;   // own the tables
  std::vector<float> data;
  ~MixedFit() {
    for (sxmc::Signal& s : base) delete s.histogram;
  }
  static sxmc::Systematic systematic(const char* name, pdfz::Systematic::Type type, double sigma, short pidx) {
    sxmc::Systematic s;
    s.name = name;
    s.type = type;
    s.observable_field_index = 0;
    s.truth_field_index = 1;
    s.means = {0.0};
    s.sigmas = {sigma};
    s.pidx = {pidx};
    return s;
  }
  void build() {
    std::mt19937_64 rng(2024);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    observables.resize(1);
    observables[0].name = "energy";
    observables[0].field_index = 0;
    observables[0].bins = 25;
    observables[0].lower = 0.0f;
    observables[0].upper = 10.0f;
    systematics = {systematic("e_scale", pdfz::Systematic::SCALE, 0.02, 0),
                   systematic("e_res", pdfz::Systematic::RESOLUTION_SCALE, 0.05, 1)};
    struct Spec {
      const char* name;
      const char* pdf;
      int n;
      float centre, width;
      double nexpected;
      bool with_systematics;
    };
    const Spec specs[] = {{"spectrum", "hist", 100000, 4.0f, 2.5f, 500.0, true},
                          {"line", "kernel", 2000, 6.0f, 0.4f, 250.0, true},
                          {"pedestal", "kernel", 800, 1.5f, 0.3f, 50.0, false}};
    for (const Spec& sp : specs) {
      std::vector<float> table;
      for (int i = 0; i < sp.n; i++) {
        const float e = sp.centre + sp.width * gauss(rng);
        table.push_back(e + 0.2f * gauss(rng));
        table.push_back(e);
      }
      sxmc::Signal s;
      s.name = sp.name;
      s.pdf = sp.pdf;
      s.source = sxmc::Source(sp.name, sources.size(), 1.0f, 0.0f, false);
      s.nexpected = sp.nexpected;
      if (s.pdf == "kernel") s.bandwidth_scale.assign(1, 1.0);
      sources.push_back(s.source);
      sxmc::build_pdfz(s, table, 2, observables, sp.with_systematics ? systematics : none);
      base.push_back(s);
      for (int e = 0; e < (int)sp.nexpected; e++) {
        const float x = table[2 * (rng() % (size_t)sp.n)];
        if (!(x >= 0.0f && x < 10.0f)) continue;
        data.push_back(x);
        data.push_back(0.0f);
      }
    }
  }
};

int run_mixed() {
  try {
    MixedFit fit;
    fit.build();
    const size_t E = fit.data.size() / 2;
    unsigned s = 1357;
    const double choice[4] = {1.0, 2.0, 3.0, 7.0};
    std::vector<double> weights(E);
    std::vector<float> repeated;
    for (size_t i = 0; i < E; i++) {
      weights[i] = choice[(SmallFit::lcg(s) >> 16) & 3u];
      for (int r = 0; r < (int)weights[i]; r++) repeated.insert(repeated.end(), fit.data.begin() + 2 * i, fit.data.begin() + 2 * i + 2);
    }
    auto walk = [&](const std::string& name, const std::function<void(sxmc::MCMC&)>& settings) {
      std::printf("%s\t", name.c_str());
      for (int which = 0; which < 3; which++) {   // unweighted, weighted, repeated: each on fresh evaluators over the shared tables
        std::vector<sxmc::Signal> signals;
        for (const sxmc::Signal& b : fit.base) signals.push_back(sxmc::share_pdfz(b));
        try {
          sxmc::MCMC m(fit.sources, signals, fit.systematics, fit.observables, 99, nullptr);
          m.optimize = false;
          settings(m);
          const sxmc::Chain c = which == 1   ? m(fit.data, weights, 600, 0.2f, false, 150)
                                : which == 2 ? m(repeated, 600, 0.2f, false, 150)
                                             : m(fit.data, 600, 0.2f, false, 150);
          std::printf("%s nrows %zu accepted %zu fnv1a %016llx form %s  ", which == 0 ? "unweighted" : which == 1 ? "weighted" : "repeated",
                      c.nrows(), c.accepted, (unsigned long long)fnv1a(c.rows.data(), c.rows.size() * 4), m.WalkFormName());
        } catch (...) {
          for (sxmc::Signal& sg : signals) delete sg.histogram;
          throw;
        }
        for (sxmc::Signal& sg : signals) delete sg.histogram;
      }
      std::printf("\n");
      std::fflush(stdout);
    };
    walk("mixed", [](sxmc::MCMC&) {});
    walk("mixed, graph_steps 16", [](sxmc::MCMC& m) { m.graph_steps = 16; });
    walk("mixed, consume off", [](sxmc::MCMC& m) { m.consume = false; });
    walk("mixed, lut_output", [](sxmc::MCMC& m) { m.lut_output = true; });
    walk("mixed, covariance", [](sxmc::MCMC& m) { m.proposal = sxmc::Proposal::COVARIANCE; });
    walk("mixed, reference_form", [](sxmc::MCMC& m) { m.reference_form = true; });
    {
      std::vector<sxmc::Signal> signals;
      for (const sxmc::Signal& b : fit.base) signals.push_back(sxmc::share_pdfz(b));
      sxmc::MCMC m(fit.sources, signals, fit.systematics, fit.observables, 99, nullptr);
      m.optimize = false;
      m.columns_in_place = true;
      std::string said = "nothing";
      try {
        m(fit.data, weights, 20, 0.2f, false, 150);
      } catch (const pdfz::Error& e) {
        said = e.msg;
      }
      std::printf("refusal: mixed, columns_in_place\t%s\n", said.c_str());
      for (sxmc::Signal& sg : signals) delete sg.histogram;
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

int run_config(const std::string& path, const std::string& dir) {
  try {
    sxmc::FitConfig fc = sxmc::load_config(path);
    for (size_t j = 0; j < fc.signals.size(); j++) {
      sxmc::build_pdfz(fc.signals[j], fc.tables[j], (int)fc.nfields, fc.observables, fc.systematics);
    }
    {
      sxmc::AsimovDataset a = sxmc::make_asimov_dataset(fc.signals, fc.systematics, fc.observables);
      write_file(dir + "/asimov_rows.f32", a.events);
      write_file(dir + "/asimov_weights.f64", a.weights);
      write_file(dir + "/asimov_nexp.f64", a.nexpected);
      sxmc::MCMC m(fc.sources, fc.signals, fc.systematics, fc.observables, 1, nullptr);
      write_file(dir + "/widths.f32", m.initial_jump_widths());
    }
    sxmc::ExperimentOptions opt;
    opt.cl = fc.confidence;
    opt.optimize = false;
    opt.asimov = fc.asimov;
    opt.proposal = fc.proposal == "covariance" ? sxmc::Proposal::COVARIANCE : sxmc::Proposal::DIAGONAL;
    opt.proposal_shrinkage = fc.proposal_shrinkage;
    size_t chains = 0;
    std::string said;
    sxmc::chain_sink() = [&](unsigned k, const sxmc::Chain& c) {
      write_file(dir + "/chain_" + std::to_string(k) + ".f32", c.rows);
      chains++;
    };
    sxmc::report_sink() = [&](unsigned, const std::string& text) { said += text; };
    std::vector<unsigned> experiments;
    for (unsigned k = 0; k < (unsigned)fc.nexperiments; k++) experiments.push_back(k);
    const std::vector<sxmc::ExperimentResult> results =
        sxmc::ensemble(experiments, fc.seed, fc.sources, fc.signals, fc.systematics, fc.observables, (unsigned)fc.nsteps,
                       fc.burnin_fraction, opt);
    std::printf("config\tasimov %d configured %u ran %zu chains %zu seed %llu nevents %zu accepted %zu\n", fc.asimov ? 1 : 0,
                (unsigned)fc.nexperiments, results.size(), chains, (unsigned long long)sxmc::experiment_seed(fc.seed, 0),
                results.empty() ? (size_t)0 : results[0].nevents, results.empty() ? (size_t)0 : results[0].accepted);
    std::printf("%s", said.c_str());
    // the runners that cannot fit one weighted data set say so
    if (fc.asimov) {
      std::string lockstep = "nothing";
      try {
        sxmc::ensemble_lockstep(experiments, fc.seed, fc.sources, fc.signals, fc.systematics, fc.observables, 20,
                                fc.burnin_fraction, 2, 1, opt);
      } catch (const pdfz::Error& e) {
        lockstep = e.msg;
      }
      std::printf("refusal: ensemble_lockstep\t%s\n", lockstep.c_str());
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("weighted_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  if (argc > 1 && std::string(argv[1]) == "--bench") return run_bench(argc > 2 ? (unsigned)std::atoi(argv[2]) : 30000u);
  if (argc > 1 && std::string(argv[1]) == "--mixed") return run_mixed();
  if (argc > 3 && std::string(argv[1]) == "--config") return run_config(argv[2], argv[3]);
  const std::string dir = argc > 1 ? argv[1] : "";
  const unsigned nsteps = 600, sync = 150;
  const float burnin = 0.2f;
  SmallFit fit;
  try {
    fit.SetUp();
    const size_t E = fit.data.size() / 3;
    unsigned s = 2468;
    const double choice[4] = {1.0, 2.0, 3.0, 7.0};
    std::vector<double> weights(E);
    std::vector<float> repeated;
    for (size_t i = 0; i < E; i++) {
      weights[i] = choice[(SmallFit::lcg(s) >> 16) & 3u];
      for (int r = 0; r < (int)weights[i]; r++) repeated.insert(repeated.end(), fit.data.begin() + 3 * i, fit.data.begin() + 3 * i + 3);
    }
    bool dumped = false;
    auto walk = [&](const std::string& name, const std::function<void(sxmc::MCMC&)>& settings) {
      std::printf("%s\t", name.c_str());
      for (int which = 0; which < 3; which++) {   // unweighted, weighted, repeated
        sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
        m.optimize = false;
        settings(m);
        const sxmc::Chain c = which == 1   ? m(fit.data, weights, nsteps, burnin, false, sync)
                              : which == 2 ? m(repeated, nsteps, burnin, false, sync)
                                           : m(fit.data, nsteps, burnin, false, sync);
        std::printf("%s nrows %zu accepted %zu fnv1a %016llx form %s  ", which == 0 ? "unweighted" : which == 1 ? "weighted" : "repeated",
                    c.nrows(), c.accepted, (unsigned long long)fnv1a(c.rows.data(), c.rows.size() * 4), m.WalkFormName());
        if (!dir.empty() && !dumped && which == 1) {
          dumped = true;
          for (size_t j = 0; j < fit.tables.size(); j++) write_file(dir + "/table" + std::to_string(j) + ".f32", fit.tables[j]);
          write_file(dir + "/data.f32", fit.data);
          write_file(dir + "/weights.f64", weights);
          write_file(dir + "/widths.f32", m.initial_jump_widths());
          write_file(dir + "/chain.f32", c.rows);
        }
      }
      std::printf("\n");
      std::fflush(stdout);
    };
    const auto cov = [](sxmc::MCMC& m) { m.proposal = sxmc::Proposal::COVARIANCE; };
    walk("defaults", [](sxmc::MCMC&) {});
    walk("graph_steps 16", [](sxmc::MCMC& m) { m.graph_steps = 16; });
    walk("reference_form", [](sxmc::MCMC& m) { m.reference_form = true; });
    walk("consume off", [](sxmc::MCMC& m) { m.consume = false; });
    walk("lookahead asked", [](sxmc::MCMC& m) { m.lookahead = true; });
    walk("covariance", cov);
    walk("covariance, graph_steps 16", [&](sxmc::MCMC& m) { cov(m); m.graph_steps = 16; });
    walk("covariance, reference_form", [&](sxmc::MCMC& m) { cov(m); m.reference_form = true; });
    auto refusal = [&](const std::string& name, const std::function<void(sxmc::MCMC&)>& settings, const std::vector<double>& w) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      settings(m);
      std::string said = "nothing";
      try {
        m(fit.data, w, 20, burnin, false, sync);
      } catch (const pdfz::Error& e) {
        said = e.msg;
      } catch (const std::exception& e) {   // (the library's own refusal, as the C++ layer's check() hands it on)
        said = e.what();
      }
      std::printf("refusal: %s\t%s\n", name.c_str(), said.c_str());
    };
    sxmc::LockstepSet set(2, nullptr);
    refusal("in a lockstep set", [&](sxmc::MCMC& m) { m.lockstep = &set; }, weights);
    refusal("columns_in_place", [](sxmc::MCMC& m) { m.columns_in_place = true; }, weights);
    refusal("a count that is not the data's", [](sxmc::MCMC&) {}, std::vector<double>(E - 1, 1.0));
    std::vector<double> bad = weights;
    bad[5] = -1.0;
    refusal("a negative weight", [](sxmc::MCMC&) {}, bad);
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.msg.c_str());
    fit.TearDown();
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "weighted_walk: %s\n", e.what());
    fit.TearDown();
    return 1;
  }
  fit.TearDown();
  return 0;
}
