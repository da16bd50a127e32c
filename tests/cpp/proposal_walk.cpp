// proposal_walk.cpp -- walks of sxmc::MCMC over the small fit (small_fit.h) with the correlated proposal
// (sxmc::Proposal::COVARIANCE), in every sequential form, for tests/test_gpu_proposal_cpp.py.  One line per case: its
// name, a tab, the chain's rows and accepted steps, a 64-bit FNV-1a hash of the bytes of Chain::rows, the form the
// walk took, the shrinkage its last factor was built with and a hash of that factor's bytes.
//   proposal_walk [DIR]
// With DIR: also writes the fit, the walk's initial widths and the first diagonal and covariance chains there as raw
// native-order files, so that the Python walker can walk the same fit from the same widths and be compared byte for
// byte: table0.f32 .. table2.f32 (rows of 4 floats), data.f32 (rows of 3), widths.f32 (P), chain_diagonal.f32 and
// chain.f32 (rows of P + 1), factor.f64 (the covariance walk's, P x P, L_ij at [j * P + i]).
// seed 7, 600 steps, burn-in fraction 0.2 (both re-tunings fall inside), sync_interval 150, optimize off (a pinned chain
// must not depend on the timing of trial launches).  Without a GPU it says so and exits 0.
//   proposal_walk --ess [nsteps]      both laws over the ESS shape of tests/test_proposal_ess_cpu.py on the device -- four
//                       floated rates over one observable (40 bins on 0-10), histograms over 200 000 samples of unit
//                       Gaussians at 3.0 / 3.15 / 7.0 / 7.15, 750 events of each, no systematic (the walk does not
//                       re-evaluate) -- seed 1, burn-in 0.2, default 30 000 steps.  One line per law: acceptance, the
//                       correlations of the two look-alike pairs, tau per rate (Sokal's automatic window, M >= 5 tau),
//                       ESS = rows / the largest tau, seconds of stepping, ESS per second.
//   proposal_walk --bench [nsteps]    steps per second of both laws: each fit warmed (2 000 steps of each law), then both
//                       laws alternating twice, graph_steps 100; the time is the walk's own host clock around its steps.
//                       Fits: "p15" -- the small fit's recipe with 13 signals of 200 000 samples, P = 15 as config 3 has
//                       (a stand-in: config 3's own tables are bench.py's) -- and "ess", the shape above.  One line per
//                       walk, as --ess.  Default 30 000 steps.
#include <algorithm>
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

// The integrated autocorrelation time 1 + 2 sum_{t <= M} rho_t of column `col`, at the smallest M with M >= 5 tau(M).
double tau_sokal(const sxmc::Chain& c, size_t col) {
  const size_t n = c.nrows();
  if (n < 2) return 1.0;
  std::vector<double> x(n);
  double mean = 0;
  for (size_t r = 0; r < n; r++) mean += c.at(r, col);
  mean /= (double)n;
  double var = 0;
  for (size_t r = 0; r < n; r++) {
    x[r] = c.at(r, col) - mean;
    var += x[r] * x[r];
  }
  if (!(var > 0)) return 1.0;
  double tau = 1.0;
  for (size_t lag = 1; lag < n; lag++) {
    double s = 0;
    for (size_t r = 0; r + lag < n; r++) s += x[r] * x[r + lag];
    tau += 2.0 * s / var;
    if ((double)lag >= 5.0 * tau) break;
  }
  return tau;
}

double correlation(const sxmc::Chain& c, size_t a, size_t b) {
  const size_t n = c.nrows();
  double ma = 0, mb = 0;
  for (size_t r = 0; r < n; r++) {
    ma += c.at(r, a);
    mb += c.at(r, b);
  }
  ma /= (double)n;
  mb /= (double)n;
  double saa = 0, sbb = 0, sab = 0;
  for (size_t r = 0; r < n; r++) {
    const double da = c.at(r, a) - ma, db = c.at(r, b) - mb;
    saa += da * da;
    sbb += db * db;
    sab += da * db;
  }
  return sab / std::sqrt(saa * sbb);
}

// A fit by the small fit's recipe: S signals of n samples (2 observables + truth + dataset; a shift and a resolution
// systematic), or, rates_only, the ESS shape: 4 signals over one observable, no systematic.
struct WalkFit {
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> signals;
  std::vector<sxmc::Systematic> systematics;
  std::vector<sxmc::Observable> observables;
  std::vector<float> data;
  ~WalkFit() {
    for (sxmc::Signal& s : signals) delete s.histogram;
  }
  void build(bool rates_only) {
    std::mt19937_64 rng(11);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const int S = rates_only ? 4 : 13, F = rates_only ? 2 : 4;
    observables.resize(rates_only ? 1 : 2);
    observables[0].field_index = 0;
    observables[0].bins = rates_only ? 40 : 12;
    observables[0].lower = 0;
    observables[0].upper = rates_only ? 10 : 1;
    if (!rates_only) {
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
    }
    const float centres[4] = {3.0f, 3.15f, 7.0f, 7.15f};
    for (int j = 0; j < S; j++) {
      const size_t n = 200000;
      std::vector<float> tab(n * (size_t)F);
      for (size_t i = 0; i < n; i++) {
        if (rates_only) {
          tab[i * 2 + 0] = centres[j] + gauss(rng);
          tab[i * 2 + 1] = 0;
        } else {
          const float t = 0.1f + 0.06f * (float)j + 0.3f * uni(rng);
          tab[i * 4 + 0] = t + 0.2f * (uni(rng) - 0.5f);
          tab[i * 4 + 1] = 2.2f * uni(rng) - 0.1f;
          tab[i * 4 + 2] = t;
          tab[i * 4 + 3] = 0;
        }
      }
      sxmc::Signal sig;
      sig.name = "sig" + std::to_string(j);
      sig.source = sxmc::Source("src" + std::to_string(j), j, 1.0f, 0.0f, false);
      sig.nexpected = rates_only ? 750 : 150;
      sxmc::build_pdfz(sig, tab, F, observables, systematics);
      signals.push_back(sig);
      sources.push_back(sig.source);
      for (int e = 0; e < (int)sig.nexpected; e++) {
        const size_t i = rng() % n;
        data.push_back(tab[i * (size_t)F + 0]);
        if (!rates_only) data.push_back(tab[i * (size_t)F + 1]);
        data.push_back(0);
      }
    }
  }
};

// One walk, one line: what --ess and --bench report.
void measured_walk(WalkFit& fit, const char* fit_name, bool covariance, unsigned nsteps, unsigned graph_steps, int repeat) {
  sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 1, nullptr);
  m.optimize = false;
  m.graph_steps = graph_steps;
  m.proposal = covariance ? sxmc::Proposal::COVARIANCE : sxmc::Proposal::DIAGONAL;
  const sxmc::Chain c = m(fit.data, nsteps, 0.2f, false, 10000);
  const size_t P = m.NumParameters();
  double worst = 1.0;
  std::string taus;
  for (size_t j = 0; j < P; j++) {
    const double tau = tau_sokal(c, j);
    worst = std::max(worst, tau);
    char buf[32];
    std::snprintf(buf, sizeof buf, "%s%.1f", j ? "," : "", tau);
    taus += buf;
  }
  const double ess = (double)c.nrows() / worst;
  std::printf("%s %s\trepeat %d steps %u form %s steps_per_second %.1f acceptance %.4f rho01 %.4f rho23 %.4f ess %.1f "
              "ess_per_second %.1f seconds %.4f tau %s\n",
              fit_name, covariance ? "covariance" : "diagonal", repeat, nsteps, m.WalkFormName(),
              (double)nsteps / c.steps_seconds, (double)c.accepted / (double)nsteps, correlation(c, 0, 1),
              correlation(c, 2, 3), ess, ess / c.steps_seconds, c.steps_seconds, taus.c_str());
  std::fflush(stdout);
}

int run_measured(bool bench, unsigned nsteps) {
  try {
    for (int which = bench ? 0 : 1; which < 2; which++) {
      WalkFit fit;
      fit.build(which == 1);
      const char* name = which == 1 ? "ess" : "p15";
      const unsigned graph_steps = bench ? 100 : 0;
      if (bench) {
        for (int law = 0; law < 2; law++) measured_walk(fit, "warm-up", law == 1, 2000, graph_steps, 0);
      }
      for (int repeat = 1; repeat <= (bench ? 2 : 1); repeat++) {
        for (int law = 0; law < 2; law++) measured_walk(fit, name, law == 1, nsteps, graph_steps, repeat);
      }
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "proposal_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "proposal_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}

template <typename T>
void write_file(const std::string& path, const std::vector<T>& v) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
  std::fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("proposal_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  if (argc > 1 && (std::string(argv[1]) == "--ess" || std::string(argv[1]) == "--bench")) {
    return run_measured(std::string(argv[1]) == "--bench", argc > 2 ? (unsigned)std::atoi(argv[2]) : 30000u);
  }
  const std::string dir = argc > 1 ? argv[1] : "";
  const unsigned nsteps = 600, sync = 150;
  const float burnin = 0.2f;
  SmallFit fit;
  try {
    fit.SetUp();
    bool dumped = false, dumped_diagonal = false;
    auto walk = [&](const std::string& name, const std::function<void(sxmc::MCMC&)>& settings) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      settings(m);
      const sxmc::Chain c = m(fit.data, nsteps, burnin, false, sync);
      double used = 0;
      const std::vector<double>& factor = m.ProposalFactor(&used);
      std::printf("%s\tnrows %zu accepted %zu fnv1a %016llx form %s passes %zu shrinkage %.17g factor %zu %016llx\n",
                  name.c_str(), c.nrows(), c.accepted, (unsigned long long)fnv1a(c.rows.data(), c.rows.size() * 4),
                  m.WalkFormName(), m.LookaheadPasses(), used, factor.size(),
                  (unsigned long long)fnv1a(factor.data(), factor.size() * 8));
      if (!dir.empty() && !dumped && m.proposal == sxmc::Proposal::COVARIANCE) {
        dumped = true;
        for (size_t j = 0; j < fit.tables.size(); j++) write_file(dir + "/table" + std::to_string(j) + ".f32", fit.tables[j]);
        write_file(dir + "/data.f32", fit.data);
        write_file(dir + "/widths.f32", m.initial_jump_widths());
        write_file(dir + "/chain.f32", c.rows);
        write_file(dir + "/factor.f64", factor);
      }
      if (!dir.empty() && !dumped_diagonal && m.proposal == sxmc::Proposal::DIAGONAL) {
        dumped_diagonal = true;
        write_file(dir + "/chain_diagonal.f32", c.rows);
      }
    };
    const auto cov = [](sxmc::MCMC& m) { m.proposal = sxmc::Proposal::COVARIANCE; };
    walk("diagonal", [](sxmc::MCMC&) {});
    walk("covariance", cov);
    walk("covariance, graph_steps 16", [&](sxmc::MCMC& m) { cov(m); m.graph_steps = 16; });
    walk("covariance, lookahead", [&](sxmc::MCMC& m) { cov(m); m.lookahead = true; });
    walk("covariance, lookahead, graph_steps 16", [&](sxmc::MCMC& m) { cov(m); m.lookahead = true; m.graph_steps = 16; });
    walk("covariance, consume off", [&](sxmc::MCMC& m) { cov(m); m.consume = false; });
    walk("covariance, reference_form", [&](sxmc::MCMC& m) { cov(m); m.reference_form = true; });
    walk("covariance, lut_output", [&](sxmc::MCMC& m) { cov(m); m.lut_output = true; });
    walk("covariance, shrinkage 0.5", [&](sxmc::MCMC& m) { cov(m); m.proposal_shrinkage = 0.5; });
    walk("covariance, shrinkage 1", [&](sxmc::MCMC& m) { cov(m); m.proposal_shrinkage = 1.0; });
    {
      // a chain of a lockstep set refuses the correlated proposal, naming the reason
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, nullptr);
      m.optimize = false;
      m.proposal = sxmc::Proposal::COVARIANCE;
      sxmc::LockstepSet set(2, nullptr);
      m.lockstep = &set;
      std::string said = "nothing";
      try {
        m(fit.data, 20, burnin, false, sync);
      } catch (const pdfz::Error& e) {
        said = e.msg;
      }
      std::printf("covariance, in a lockstep set\t%s\n", said.c_str());
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "proposal_walk: %s\n", e.msg.c_str());
    fit.TearDown();
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "proposal_walk: %s\n", e.what());
    fit.TearDown();
    return 1;
  }
  fit.TearDown();
  return 0;
}
