// constraint_walk.cpp -- walks of sxmc::MCMC with CORRELATED GAUSSIAN CONSTRAINTS (MCMC::constraint_correlation) in every
// sequential form, for tests/test_gpu_constraint_cpp.py.  One line per case: its name, a tab, the chain's rows and accepted
// steps, a 64-bit FNV-1a hash of the bytes of Chain::rows, the form the walk took, the look-ahead passes it launched and a
// hash of the whitening matrix it went through (size 0 without one).
//   constraint_walk [DIR]
// The small fit (small_fit.h: P = 5, the shift's and the resolution's constraints are parameters 3 and 4), seed 7, 600
// steps, burn-in fraction 0.2 (both re-tunings fall inside), sync_interval 150, optimize off.  Three constraint laws:
// "none" (no matrix), "identity" (rho = I: W = I, which must give the bytes of "none") and "correlated" (rho_34 = -0.6),
// each in the consuming form, replayed from graphs of 16 steps, asked with lookahead (with and without graphs), batched,
// in the reference's launches and with the lookup table; then with the covariance proposal, with weighted events and
// with a weighted histogram member.  With DIR: also writes the fit, the walk's initial widths, the correlated chain and its
// whitening matrix there as raw native-order files (table0.f32 .. table2.f32, data.f32, widths.f32, chain_none.f32,
// chain.f32, whitening.f64), so that the Python walker can walk the same fit and be compared byte for byte.  Then the
// refusals: a chain of a lockstep set, a matrix that is not positive definite, one of the wrong size.
//   constraint_walk --mixed          the same three laws over a mixed histogram + kernel-density fit (P = 5, the scale's and
//                       the resolution's constraints), in the reference's launches, the MIXED form, with graphs, with
//                       columns_in_place and asked with lookahead.
//   constraint_walk --bench [nsteps] steps per second at the "p15" stand-in shape of proposal_walk (13 signals of 200 000
//                       samples, P = 15; consuming form, graphs of 100 steps): warmed (2 000 steps of each case), then
//                       the three cases alternating twice: no matrix, W = I, and a dense 15 x 15 W.  Default 30 000 steps.
// Without a GPU it says so and exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
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

template <typename T>
void write_file(const std::string& path, const std::vector<T>& v) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
  std::fclose(f);
}

std::vector<double> identity(size_t P) {
  std::vector<double> rho(P * P, 0.0);
  for (size_t i = 0; i < P; i++) rho[i * P + i] = 1.0;
  return rho;
}

// rho = I with rho_ab = rho_ba = value
std::vector<double> pair(size_t P, size_t a, size_t b, double value) {
  std::vector<double> rho = identity(P);
  rho[a * P + b] = rho[b * P + a] = value;
  return rho;
}

void report(const std::string& name, sxmc::MCMC& m, const sxmc::Chain& c) {
  const std::vector<double>& W = m.ConstraintWhitening();
  std::printf("%s\tnrows %zu accepted %zu fnv1a %016llx form %s passes %zu whitening %zu %016llx\n", name.c_str(),
              c.nrows(), c.accepted, (unsigned long long)fnv1a(c.rows.data(), c.rows.size() * 4), m.WalkFormName(),
              m.LookaheadPasses(), W.size(), (unsigned long long)fnv1a(W.data(), W.size() * 8));
  std::fflush(stdout);
}

std::string refusal(const std::function<void()>& f) {
  try {
    f();
  } catch (const pdfz::Error& e) {
    return e.msg;
  } catch (const std::exception& e) {
    return e.what();
  }
  return "nothing";
}

struct Form {
  const char* name;
  std::function<void(sxmc::MCMC&)> set;
};

const std::vector<Form>& forms() {
  static const std::vector<Form> f = {
      {"consuming", [](sxmc::MCMC&) {}},
      {"graph_steps 16", [](sxmc::MCMC& m) { m.graph_steps = 16; }},
      {"lookahead", [](sxmc::MCMC& m) { m.lookahead = true; }},
      {"lookahead, graph_steps 16", [](sxmc::MCMC& m) { m.lookahead = true; m.graph_steps = 16; }},
      {"consume off", [](sxmc::MCMC& m) { m.consume = false; }},
      {"reference_form", [](sxmc::MCMC& m) { m.reference_form = true; }},
      {"lut_output", [](sxmc::MCMC& m) { m.lut_output = true; }}};
  return f;
}

int run_small(const std::string& dir) {
  const unsigned nsteps = 600, sync = 150;
  const float burnin = 0.2f;
  SmallFit fit;
  int rc = 0;
  try {
    fit.SetUp();
    const size_t P = 5;
    struct Law {
      const char* name;
      std::vector<double> rho;
    };
    const std::vector<Law> laws = {{"none", {}}, {"identity", identity(P)}, {"correlated", pair(P, 3, 4, -0.6)}};
    std::vector<double> weights(fit.data.size() / 3);
    for (size_t i = 0; i < weights.size(); i++) weights[i] = 0.25 * (double)(1 + i % 7);
    bool dumped = false, dumped_none = false;
    auto walk = [&](const std::string& name, const std::vector<double>& rho, const std::function<void(sxmc::MCMC&)>& set,
                    bool weighted) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      m.constraint_correlation = rho;
      set(m);
      const sxmc::Chain c = weighted ? m(fit.data, weights, nsteps, burnin, false, sync) : m(fit.data, nsteps, burnin, false, sync);
      report(name, m, c);
      if (!dir.empty() && !dumped && name == "correlated, consuming") {
        dumped = true;
        for (size_t j = 0; j < fit.tables.size(); j++) write_file(dir + "/table" + std::to_string(j) + ".f32", fit.tables[j]);
        write_file(dir + "/data.f32", fit.data);
        write_file(dir + "/widths.f32", m.initial_jump_widths());
        write_file(dir + "/chain.f32", c.rows);
        write_file(dir + "/whitening.f64", m.ConstraintWhitening());
      }
      if (!dir.empty() && !dumped_none && name == "none, consuming") {
        dumped_none = true;
        write_file(dir + "/chain_none.f32", c.rows);
      }
    };
    for (const Law& law : laws)
      for (const Form& f : forms()) walk(std::string(law.name) + ", " + f.name, law.rho, f.set, false);
    // the covariance proposal, weighted events: the forms that record and the one asked with lookahead
    const std::vector<Form> few = {forms()[0], forms()[1], forms()[2]};
    for (const Law& law : laws) {
      for (const Form& f : few) {
        walk(std::string(law.name) + ", covariance, " + f.name, law.rho,
             [&](sxmc::MCMC& m) { f.set(m); m.proposal = sxmc::Proposal::COVARIANCE; }, false);
        walk(std::string(law.name) + ", weighted events, " + f.name, law.rho, f.set, true);
      }
    }
    // a weighted histogram member: signal 1 rebuilt with multiplicities 1 + i % 3
    {
      sxmc::Signal& old = fit.signals[1];
      sxmc::Signal sig;
      sig.name = old.name;
      sig.source = old.source;
      sig.nexpected = old.nexpected;
      sig.multiplicities.resize(fit.tables[1].size() / 4);
      for (size_t i = 0; i < sig.multiplicities.size(); i++) sig.multiplicities[i] = 1u + (unsigned)(i % 3);
      sxmc::build_pdfz(sig, fit.tables[1], 4, fit.observables, fit.systematics);
      delete old.histogram;
      old = sig;
    }
    for (const Law& law : laws)
      for (const Form& f : few) walk(std::string(law.name) + ", sample weights, " + f.name, law.rho, f.set, false);

    // refusals
    {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      m.constraint_correlation = pair(P, 3, 4, -0.6);
      sxmc::LockstepSet set(2, nullptr);
      m.lockstep = &set;
      std::printf("correlated, in a lockstep set\t%s\n", refusal([&] { m(fit.data, 20, burnin, false, sync); }).c_str());
    }
    {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.constraint_correlation = pair(P, 3, 4, 1.0);
      std::printf("not positive definite\t%s\n", refusal([&] { m(fit.data, 20, burnin, false, sync); }).c_str());
      m.constraint_correlation = pair(P, 0, 4, 0.5);   // (source 0 has no constraint)
      std::printf("unconstrained\t%s\n", refusal([&] { m(fit.data, 20, burnin, false, sync); }).c_str());
      m.constraint_correlation = identity(4);
      std::printf("wrong size\t%s\n", refusal([&] { m(fit.data, 20, burnin, false, sync); }).c_str());
      m.constraint_correlation.clear();
      const sxmc::Chain c = m(fit.data, 20, burnin, false, sync);   // (the chain is usable after the refusals)
      std::printf("after the refusals\tnrows %zu\n", c.nrows());
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.msg.c_str());
    rc = 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.what());
    rc = 1;
  }
  fit.TearDown();
  return rc;
}

// ---------------------------------------------------------------------------------------------- the mixed fit
struct MixedFit {
  std::vector<sxmc::Observable> observables;
  std::vector<sxmc::Systematic> systematics, none;
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> base;   // own the tables
  std::vector<float> data;
  ~MixedFit() {
    for (sxmc::Signal& s : base) delete s.histogram;
  }
};

sxmc::Systematic systematic(const char* name, pdfz::Systematic::Type type, double sigma, short pidx) {
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

void build(MixedFit& fit) {
  std::mt19937_64 rng(2025);
  std::normal_distribution<float> gauss(0.0f, 1.0f);
  fit.observables.resize(1);
  fit.observables[0].name = "energy";
  fit.observables[0].field_index = 0;
  fit.observables[0].bins = 25;
  fit.observables[0].lower = 0.0f;
  fit.observables[0].upper = 10.0f;
  fit.systematics = {systematic("e_scale", pdfz::Systematic::SCALE, 0.02, 0),
                     systematic("e_res", pdfz::Systematic::RESOLUTION_SCALE, 0.05, 1)};
  struct Spec {
    const char* name;
    const char* pdf;
    int n;
    float centre, width;
    double nexpected;
    bool with_systematics;
  };
  const Spec specs[] = {{"spectrum", "hist", 50000, 4.0f, 2.5f, 400.0, true},
                        {"line", "kernel", 1500, 6.0f, 0.4f, 200.0, true},
                        {"pedestal", "kernel", 600, 1.5f, 0.3f, 50.0, false}};
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
    s.source = sxmc::Source(sp.name, fit.sources.size(), 1.0f, 0.0f, false);
    s.nexpected = sp.nexpected;
    if (s.pdf == "kernel") s.bandwidth_scale.assign(1, 1.0);
    fit.sources.push_back(s.source);
    sxmc::build_pdfz(s, table, 2, fit.observables, sp.with_systematics ? fit.systematics : fit.none);
    fit.base.push_back(s);
    for (int e = 0; e < (int)sp.nexpected; e++) {
      const float x = table[2 * (rng() % (size_t)sp.n)];
      if (!(x >= 0.0f && x < 10.0f)) continue;
      fit.data.push_back(x);
      fit.data.push_back(0.0f);
    }
  }
}

int run_mixed() {
  struct Setting {
    const char* name;
    bool reference_form;
    unsigned graph_steps;
    bool in_place, lookahead;
  };
  const Setting settings[] = {{"reference_form", true, 0, false, false},
                              {"mixed", false, 0, false, false},
                              {"graph_steps 16", false, 16, false, false},
                              {"columns_in_place", false, 0, true, false},
                              {"columns_in_place, graph_steps 16", false, 16, true, false},
                              {"lookahead", false, 0, false, true}};
  try {
    MixedFit fit;
    build(fit);
    const size_t P = 5;
    const std::pair<const char*, std::vector<double>> laws[] = {
        {"none", {}}, {"identity", identity(P)}, {"correlated", pair(P, 3, 4, 0.7)}};
    for (const auto& law : laws) {
      for (const Setting& st : settings) {
        std::vector<sxmc::Signal> signals;
        for (const sxmc::Signal& b : fit.base) signals.push_back(sxmc::share_pdfz(b));
        try {
          sxmc::MCMC m(fit.sources, signals, fit.systematics, fit.observables, 99, nullptr);
          m.optimize = false;
          m.constraint_correlation = law.second;
          m.reference_form = st.reference_form;
          m.graph_steps = st.graph_steps;
          m.columns_in_place = st.in_place;
          m.lookahead = st.lookahead;
          const sxmc::Chain c = m(fit.data, 300, 0.2f, false, 100);
          report(std::string(law.first) + ", " + st.name, m, c);
        } catch (...) {
          for (sxmc::Signal& s : signals) delete s.histogram;
          throw;
        }
        for (sxmc::Signal& s : signals) delete s.histogram;
      }
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------- the bench
// proposal_walk's "p15" recipe: 13 signals of 200 000 samples over two observables, a shift and a resolution systematic.
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
    observables[0].field_index = 0;
    observables[0].bins = 12;
    observables[0].lower = 0;
    observables[0].upper = 1;
    observables[1].field_index = 1;
    observables[1].bins = 9;
    observables[1].lower = 0;
    observables[1].upper = 2;
    systematics.resize(2);
    systematics[0].name = "shift";
    systematics[0].type = pdfz::Systematic::SHIFT;
    systematics[0].observable_field_index = 1;
    systematics[0].means = {0.0};
    systematics[0].sigmas = {0.05};
    systematics[0].pidx = {0};
    systematics[1].name = "res";
    systematics[1].type = pdfz::Systematic::RESOLUTION_SCALE;
    systematics[1].observable_field_index = 0;
    systematics[1].truth_field_index = 2;
    systematics[1].means = {0.0};
    systematics[1].sigmas = {0.1};
    systematics[1].pidx = {1};
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
      // (every rate carries a constraint here, so that a dense 15 x 15 matrix is accepted)
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.5f, false);
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
    const size_t P = 15;
    // dense and well conditioned: rho_ij = 0.3^|i - j|
    std::vector<double> dense(P * P);
    for (size_t i = 0; i < P; i++)
      for (size_t j = 0; j < P; j++) dense[i * P + j] = i == j ? 1.0 : std::pow(0.3, std::fabs((double)i - (double)j));
    const std::pair<const char*, std::vector<double>> cases[] = {{"none", {}}, {"identity", identity(P)}, {"dense", dense}};
    auto walk = [&](const char* label, const std::pair<const char*, std::vector<double>>& cs, unsigned steps, int repeat) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 1, nullptr);
      m.optimize = false;
      m.graph_steps = 100;
      m.constraint_correlation = cs.second;
      const sxmc::Chain c = m(fit.data, steps, 0.2f, false, 10000);
      std::printf("%s %s\trepeat %d steps %u form %s steps_per_second %.1f acceptance %.4f seconds %.4f\n", label, cs.first,
                  repeat, steps, m.WalkFormName(), (double)steps / c.steps_seconds, (double)c.accepted / (double)steps,
                  c.steps_seconds);
      std::fflush(stdout);
    };
    for (const auto& cs : cases) walk("warm-up", cs, 2000, 0);
    for (int repeat = 1; repeat <= 2; repeat++)
      for (const auto& cs : cases) walk("p15", cs, nsteps, repeat);
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "constraint_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("constraint_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--bench") return run_bench(argc > 2 ? (unsigned)std::atoi(argv[2]) : 30000u);
  if (mode == "--mixed") return run_mixed();
  return run_small(mode);
}
