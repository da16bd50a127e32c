// mixed_walk.cpp -- sxmc::MCMC over fits that mix histogram and kernel-density signals, in every form such a walk can
// take, for tests/test_gpu_mixed_walk.py and for the measurements of the README's "Mixed walks".
//
// mixed_walk            the test fit -- one observable (energy 0-10, 25 bins) with a truth field; `spectrum`: histogram,
//                       2e5 samples, scale + resolution; `line`: kernel density, 3 000 samples, the same two systematics;
//                       `pedestal`: kernel density, 1 000 samples, no systematic; about 900 events -- walked 3 000 steps
//                       (burn-in 0.1, sync_interval 1000, one seed) with eight settings, each on fresh evaluators that
//                       share the tables: reference_form, defaults, lut_output, graph_steps = 16, consume = false, the
//                       defaults once more with `line`'s bandwidth scale at 1.01, and columns_in_place without and with
//                       graph_steps = 16.  One JSON line: per walk the form,
//                       rows, accepted count, a hash of the recorded bytes, whether they are the first walk's bytes, and
//                       the evaluation counts of `line` and `pedestal`.  Exit status 0 when the walks ran.
// mixed_walk --big      the same eight walks over a histogram of 40 x 40 x 40 bins, beyond LDS: the group counts the event
//                       bins only, and the in-place look-ups read those counters.
// mixed_walk --bench a|b [nsteps]   steps per second of the reference form, the mixed form and the mixed form with
//                       columns_in_place: each warmed, then timed twice, alternating; the time is the walk's own host clock
//                       around its steps, ending in a wait for its stream, set-up excluded.  a: the test fit;
//                       b: 2 observables (50 x 30 bins), 8 histogram signals of 4e6 samples, a kernel signal of 8 192
//                       samples with shift + scale + resolution floated, one of 4 096 with none, 5e4 events,
//                       graph_steps 100.  Default 20 000 steps.
// Without a GPU it says so and exits 0.
#include <sxmc/pdfz.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/mcmc.h"

namespace {

struct Fit {
  int F = 2;
  std::vector<sxmc::Observable> observables;
  std::vector<sxmc::Systematic> systematics, none;
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> base;        // own the tables
  std::vector<float> data;
  ~Fit() {
    for (sxmc::Signal& s : base) delete s.histogram;
  }
};

sxmc::Systematic systematic(const char* name, pdfz::Systematic::Type type, size_t obs, size_t truth, double sigma, short pidx) {
  sxmc::Systematic s;
  s.name = name;
  s.type = type;
  s.observable_field_index = obs;
  s.truth_field_index = truth;
  s.means = {0.0};
  s.sigmas = {sigma};
  s.pidx = {pidx};
  return s;
}

void add_signal(Fit& fit, const char* name, const char* pdf, double nexpected, const std::vector<float>& table,
                bool with_systematics, double bandwidth_scale = 1.0) {
  sxmc::Signal s;
  s.name = name;
  s.pdf = pdf;
  s.source = sxmc::Source(name, fit.sources.size(), 1.0f, 0.0f, false);
  s.nexpected = nexpected;
  if (s.pdf == "kernel") s.bandwidth_scale.assign(fit.observables.size(), bandwidth_scale);
  fit.sources.push_back(s.source);
  sxmc::build_pdfz(s, table, fit.F, fit.observables, with_systematics ? fit.systematics : fit.none);
  fit.base.push_back(s);
}

// The test fit.  nbins3: > 0 makes it three observables of that many bins each (a histogram beyond LDS).
void build_test_fit(Fit& fit, double line_bandwidth_scale, int nbins3) {
  std::mt19937_64 rng(7);
  std::normal_distribution<float> gauss(0.0f, 1.0f);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  const int D = nbins3 > 0 ? 3 : 1;
  fit.F = D + 1;   // observables, then the true energy
  fit.observables.resize((size_t)D);
  for (int d = 0; d < D; d++) {
    fit.observables[(size_t)d].name = d == 0 ? "energy" : d == 1 ? "radius" : "angle";
    fit.observables[(size_t)d].field_index = (size_t)d;
    fit.observables[(size_t)d].bins = nbins3 > 0 ? (size_t)nbins3 : 25;
    fit.observables[(size_t)d].lower = 0.0f;
    fit.observables[(size_t)d].upper = d == 0 ? 10.0f : 1.0f;
  }
  fit.systematics = {systematic("e_scale", pdfz::Systematic::SCALE, 0, 0, 0.02, 0),
                     systematic("e_res", pdfz::Systematic::RESOLUTION_SCALE, 0, (size_t)D, 0.05, 1)};
  auto table = [&](int n, auto truth) {
    std::vector<float> t;
    for (int i = 0; i < n; i++) {
      const float e = truth();
      t.push_back(e + 0.2f * gauss(rng));
      for (int d = 1; d < D; d++) t.push_back(uni(rng));
      t.push_back(e);
    }
    return t;
  };
  const std::vector<float> flat = table(200000, [&] { return 10.0f * uni(rng) * uni(rng); });
  const std::vector<float> line = table(3000, [&] { return 6.0f + 0.4f * gauss(rng); });
  const std::vector<float> pedestal = table(1000, [&] { return 1.5f + 0.3f * gauss(rng); });
  add_signal(fit, "spectrum", "hist", 600.0, flat, true);
  add_signal(fit, "line", "kernel", 250.0, line, true, line_bandwidth_scale);
  add_signal(fit, "pedestal", "kernel", 50.0, pedestal, false);
  const std::vector<float>* tables[3] = {&flat, &line, &pedestal};
  for (int j = 0; j < 3; j++) {
    for (int e = 0; e < (int)fit.base[(size_t)j].nexpected; e++) {
      const size_t i = rng() % (tables[j]->size() / (size_t)fit.F);
      const float x = (*tables[j])[i * (size_t)fit.F];
      if (!(x >= 0.0f && x < 10.0f)) continue;
      for (int d = 0; d < D; d++) fit.data.push_back((*tables[j])[i * (size_t)fit.F + (size_t)d]);
      fit.data.push_back(0.0f);
    }
  }
}

// The larger shape of the measurements (b).
void build_bench_fit(Fit& fit) {
  std::mt19937_64 rng(11);
  std::normal_distribution<float> gauss(0.0f, 1.0f);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  fit.F = 3;   // energy, radius, true energy
  fit.observables.resize(2);
  fit.observables[0].name = "energy";
  fit.observables[0].field_index = 0;
  fit.observables[0].bins = 50;
  fit.observables[0].lower = 0.0f;
  fit.observables[0].upper = 10.0f;
  fit.observables[1].name = "radius";
  fit.observables[1].field_index = 1;
  fit.observables[1].bins = 30;
  fit.observables[1].lower = 0.0f;
  fit.observables[1].upper = 1.0f;
  fit.systematics = {systematic("e_shift", pdfz::Systematic::SHIFT, 0, 0, 0.02, 0),
                     systematic("e_scale", pdfz::Systematic::SCALE, 0, 0, 0.01, 1),
                     systematic("e_res", pdfz::Systematic::RESOLUTION_SCALE, 0, 2, 0.03, 2)};
  auto table = [&](size_t n, float centre, float width) {
    std::vector<float> t;
    t.reserve(n * 3);
    for (size_t i = 0; i < n; i++) {
      const float e = centre + width * gauss(rng);
      t.push_back(e + 0.25f * gauss(rng));
      t.push_back(std::sqrt(uni(rng)));
      t.push_back(e);
    }
    return t;
  };
  std::vector<std::vector<float>> tables;
  for (int j = 0; j < 8; j++) {
    tables.push_back(table(4000000, 1.0f + 1.0f * (float)j, 0.8f + 0.2f * (float)j));
    add_signal(fit, ("background" + std::to_string(j)).c_str(), "hist", 6000.0, tables.back(), true);
  }
  tables.push_back(table(8192, 6.5f, 0.3f));
  add_signal(fit, "line", "kernel", 1500.0, tables.back(), true);
  tables.push_back(table(4096, 2.0f, 0.5f));
  add_signal(fit, "pedestal", "kernel", 500.0, tables.back(), false);
  for (size_t j = 0; j < tables.size(); j++) {
    for (int e = 0; e < (int)fit.base[j].nexpected; e++) {
      const size_t i = rng() % (tables[j].size() / 3);
      const float x = tables[j][i * 3], r = tables[j][i * 3 + 1];
      if (!(x >= 0.0f && x < 10.0f && r >= 0.0f && r < 1.0f)) continue;
      fit.data.push_back(x);
      fit.data.push_back(r);
      fit.data.push_back(0.0f);
    }
  }
}

struct Setting {
  const char* name;
  bool reference_form, lut_output, consume;
  unsigned graph_steps;
  bool in_place = false;
};

struct Result {
  sxmc::Chain chain;
  std::string form;
  unsigned long long line_evals = 0, pedestal_evals = 0;
  int fill_launches = 0;   // launches of the group's fill, as its launch plan lists them
};

unsigned long long evaluations(const sxmc::Signal& s) {
  pdfz::EvalKernel* k = dynamic_cast<pdfz::EvalKernel*>(s.histogram);
  return k ? k->EvaluationCount() : 0;
}

// One walk on fresh evaluators over the fit's tables.
Result walk(Fit& fit, const Setting& st, unsigned nsteps, unsigned sync_interval) {
  std::vector<sxmc::Signal> signals;
  for (const sxmc::Signal& b : fit.base) signals.push_back(sxmc::share_pdfz(b));
  Result r;
  try {
    sxmc::MCMC mcmc(fit.sources, signals, fit.systematics, fit.observables, 4321, nullptr);
    mcmc.reference_form = st.reference_form;
    mcmc.lut_output = st.lut_output;
    mcmc.consume = st.consume;
    mcmc.graph_steps = st.graph_steps;
    mcmc.columns_in_place = st.in_place;
    r.chain = mcmc(fit.data, nsteps, 0.1f, false, sync_interval);
    r.form = mcmc.WalkFormName();
    const std::string plan = mcmc.LaunchPlan();
    for (size_t at = plan.find("launch "); at != std::string::npos; at = plan.find("launch ", at + 1)) {
      if (at == 0 || plan[at - 1] == '\n') r.fill_launches++;
    }
    for (const sxmc::Signal& s : signals) {
      if (s.name == "line") r.line_evals = evaluations(s);
      if (s.name == "pedestal") r.pedestal_evals = evaluations(s);
    }
  } catch (...) {
    for (sxmc::Signal& s : signals) delete s.histogram;
    throw;
  }
  for (sxmc::Signal& s : signals) delete s.histogram;
  return r;
}

unsigned long long fnv1a(const std::vector<float>& v) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(float); i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

int run_test(bool big) {
  const unsigned nsteps = 3000;
  const Setting settings[] = {{"reference_form", true, false, true, 0}, {"defaults", false, false, true, 0},
                              {"lut_output", false, true, true, 0},     {"graph_steps_16", false, false, true, 16},
                              {"no_consume", false, false, false, 0},   {"bandwidth_1.01", false, false, true, 0},
                              {"in_place", false, false, true, 0, true}, {"in_place_graph_16", false, false, true, 16, true}};
  std::string out = "{\"nsteps\": 3000, \"walks\": [";
  Result first;
  for (size_t w = 0; w < sizeof settings / sizeof settings[0]; w++) {
    Fit fit;   // (the bandwidth walk: other tables' bandwidths; the others could share one, but a fit is cheap)
    build_test_fit(fit, w == 5 ? 1.01 : 1.0, big ? 40 : 0);
    Result r = walk(fit, settings[w], nsteps, 1000);
    if (w == 0) first = r;
    const bool same = r.chain.rows.size() == first.chain.rows.size() &&
                      std::memcmp(r.chain.rows.data(), first.chain.rows.data(), r.chain.rows.size() * sizeof(float)) == 0 &&
                      r.chain.accepted == first.chain.accepted;
    size_t finite = 0;
    const size_t col = r.chain.names.size() - 1;
    for (size_t q = 0; q < r.chain.nrows(); q++) finite += std::isfinite(r.chain.at(q, col)) ? 1 : 0;
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "%s{\"setting\": \"%s\", \"form\": \"%s\", \"rows\": %zu, \"finite_nll_rows\": %zu, \"accepted\": %zu, "
                  "\"hash\": \"%016llx\", \"same_as_first\": %s, \"line_evaluations\": %llu, \"pedestal_evaluations\": %llu, "
                  "\"events\": %zu}",
                  w ? ", " : "", settings[w].name, r.form.c_str(), r.chain.nrows(), finite, r.chain.accepted,
                  fnv1a(r.chain.rows), same ? "true" : "false", r.line_evals, r.pedestal_evals,
                  fit.data.size() / (size_t)fit.F);
    out += buf;
  }
  std::printf("%s]}\n", out.c_str());
  return 0;
}

int run_bench(const std::string& shape, unsigned nsteps) {
  Fit fit;
  unsigned graph_steps = 0;
  if (shape == "b") {
    build_bench_fit(fit);
    graph_steps = 100;
  } else {
    build_test_fit(fit, 1.0, 0);
  }
  const Setting forms[3] = {{"reference", true, false, true, 0},
                            {"mixed", false, false, true, graph_steps},
                            {"mixed_in_place", false, false, true, graph_steps, true}};
  double rate[3][2];
  int fill_launches = 0;
  for (int f = 0; f < 3; f++) (void)walk(fit, forms[f], std::min(nsteps, 2000u), 1000);   // warm
  for (int rep = 0; rep < 2; rep++) {
    for (int f = 0; f < 3; f++) {
      const Result r = walk(fit, forms[f], nsteps, 10000);
      rate[f][rep] = (double)nsteps / r.chain.steps_seconds;
      if (f == 1) fill_launches = r.fill_launches;
    }
  }
  std::string out = "{\"shape\": \"" + shape + "\", \"nsteps\": " + std::to_string(nsteps) +
                    ", \"events\": " + std::to_string(fit.data.size() / (size_t)fit.F) + ", \"fill_launches\": " +
                    std::to_string(fill_launches) + ", \"steps_per_second\": {";
  for (int f = 0; f < 3; f++) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s\"%s\": [%.1f, %.1f]", f ? ", " : "", forms[f].name, rate[f][0], rate[f][1]);
    out += buf;
  }
  std::printf("%s}}\n", out.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("mixed_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  try {
    if (argc > 2 && std::string(argv[1]) == "--bench") {
      return run_bench(argv[2], argc > 3 ? (unsigned)std::atoi(argv[3]) : 20000u);
    }
    return run_test(argc > 1 && std::string(argv[1]) == "--big");
  } catch (const pdfz::Error& e) {
    std::printf("mixed_walk: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("mixed_walk: %s\n", e.what());
  }
  return 1;
}
