// proposal_mixed_walk.cpp -- sxmc::MCMC with the correlated proposal over a fit that mixes a histogram signal with
// kernel-density signals, in every form such a walk can take, for tests/test_gpu_proposal_mixed.py.
//
// The fit: one observable (energy 0-10, 25 bins) and a truth field; `spectrum`: a histogram over 100 000 samples with a
// scale and a resolution systematic; `line`: kernel density over 2 000 samples with the same two systematics; `pedestal`:
// kernel density over 800 samples, no systematic; about 800 events.  Five parameters, all floating.
// 600 steps, burn-in 0.2 (both re-tunings fall inside), sync_interval 150, seed 99, each walk on fresh evaluators that
// share the tables.  One line per walk: its name, a tab, rows, accepted steps, a hash of the chain's bytes, the form,
// the off-diagonal entries of the last factor that are not zero.
//   diagonal / reference_form   the reference's launches with the diagonal proposal
//   covariance / ...            reference_form (the group-less launch point with the factor), the mixed form (the columns
//                               step end), lut_output, graph_steps = 16, consume = false (the plain step end),
//                               columns_in_place without and with graph_steps = 16, and asked with lookahead
// Without a GPU it says so and exits 0.
#include <sxmc/pdfz.h>

#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/mcmc.h"

namespace {

struct Fit {
  std::vector<sxmc::Observable> observables;
  std::vector<sxmc::Systematic> systematics, none;
  std::vector<sxmc::Source> sources;
  std::vector<sxmc::Signal> base;   // own the tables
  std::vector<float> data;
  ~Fit() {
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

void build(Fit& fit) {
  std::mt19937_64 rng(2024);
  std::normal_distribution<float> gauss(0.0f, 1.0f);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
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
  (void)uni;
}

struct Setting {
  const char* name;
  bool covariance, reference_form, lut_output, consume;
  unsigned graph_steps;
  bool in_place, lookahead;
};

unsigned long long fnv1a(const void* data, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

void walk(Fit& fit, const Setting& st) {
  std::vector<sxmc::Signal> signals;
  for (const sxmc::Signal& b : fit.base) signals.push_back(sxmc::share_pdfz(b));
  try {
    sxmc::MCMC m(fit.sources, signals, fit.systematics, fit.observables, 99, nullptr);
    m.optimize = false;
    m.proposal = st.covariance ? sxmc::Proposal::COVARIANCE : sxmc::Proposal::DIAGONAL;
    m.reference_form = st.reference_form;
    m.lut_output = st.lut_output;
    m.consume = st.consume;
    m.graph_steps = st.graph_steps;
    m.columns_in_place = st.in_place;
    m.lookahead = st.lookahead;
    const sxmc::Chain c = m(fit.data, 600, 0.2f, false, 150);
    const std::vector<double>& L = m.ProposalFactor();
    const size_t P = m.NumParameters();
    size_t off_diagonal = 0;
    for (size_t k = 0; k < L.size(); k++) off_diagonal += (k / P != k % P && L[k] != 0.0) ? 1 : 0;
    std::printf("%s\tnrows %zu accepted %zu fnv1a %016llx form %s off_diagonal %zu parameters %zu\n", st.name, c.nrows(),
                c.accepted, fnv1a(c.rows.data(), c.rows.size() * sizeof(float)), m.WalkFormName(), off_diagonal, P);
  } catch (...) {
    for (sxmc::Signal& s : signals) delete s.histogram;
    throw;
  }
  for (sxmc::Signal& s : signals) delete s.histogram;
}

}  // namespace

int main() {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("proposal_mixed_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  const Setting settings[] = {{"diagonal, reference_form", false, true, false, true, 0, false, false},
                              {"covariance, reference_form", true, true, false, true, 0, false, false},
                              {"covariance, mixed", true, false, false, true, 0, false, false},
                              {"covariance, lut_output", true, false, true, true, 0, false, false},
                              {"covariance, graph_steps 16", true, false, false, true, 16, false, false},
                              {"covariance, consume off", true, false, false, false, 0, false, false},
                              {"covariance, columns_in_place", true, false, false, true, 0, true, false},
                              {"covariance, columns_in_place, graph_steps 16", true, false, false, true, 16, true, false},
                              {"covariance, lookahead", true, false, false, true, 0, false, true}};
  try {
    Fit fit;
    build(fit);
    for (const Setting& st : settings) walk(fit, st);
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "proposal_mixed_walk: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "proposal_mixed_walk: %s\n", e.what());
    return 1;
  }
  return 0;
}
