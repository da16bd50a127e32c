// kde_cutoff_fit.cpp -- a mixed fit whose kernel-density signal carries "bandwidth_cutoff", from a configuration file
// through the C++ layers: sxmc::load_config, build_pdfz (which applies the cutoff), share_pdfz (shared evaluators copy
// it), then sxmc::MCMC over events drawn from the tables -- once in the reference's own call sequence and once in the
// default (mixed) form, on fresh shared evaluators each.
// Prints one JSON line: per kernel signal its name and the cutoff its evaluator and a shared one report; per walk its
// form, rows, accepted steps and the kernel signals' visited / possible tiles after it; and whether the two chains are
// the same bytes.  Without a GPU it says so and exits 0.
// Usage: kde_cutoff_fit <config.json>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/config.h"
#include "../../sxmc_amd/include/sxmc/mcmc.h"

static void print_cutoff(double R) {
  if (std::isinf(R)) std::printf("\"inf\"");
  else std::printf("%.17g", R);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: kde_cutoff_fit <config.json>\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("kde_cutoff_fit: no GPU device, nothing to run\n");
    return 0;
  }
  std::vector<sxmc::Signal> base;
  int status = 1;
  try {
    sxmc::FitConfig fc = sxmc::load_config(argv[1]);
    base = fc.signals;
    for (size_t j = 0; j < base.size(); j++)
      sxmc::build_pdfz(base[j], fc.tables[j], (int)fc.nfields, fc.observables, fc.systematics);
    const size_t D = fc.observables.size(), F = fc.nfields;
    // events: rows of the tables inside the domain, nexpected of each signal
    std::vector<float> lower(D), upper(D);
    for (const sxmc::Observable& o : fc.observables) {
      lower.at(o.field_index) = o.lower;
      upper.at(o.field_index) = o.upper;
    }
    std::mt19937_64 rng(17);
    std::vector<float> data;
    for (size_t j = 0; j < base.size(); j++) {
      const std::vector<float>& t = fc.tables[j];
      for (int e = 0; e < (int)base[j].nexpected; e++) {
        const size_t i = rng() % (t.size() / F);
        bool in = true;
        for (size_t d = 0; d < D; d++) in = in && t[i * F + d] >= lower[d] && t[i * F + d] < upper[d];
        if (!in) continue;
        for (size_t d = 0; d < D; d++) data.push_back(t[i * F + d]);
        data.push_back((float)base[j].dataset);
      }
    }
    std::printf("{\"kernels\": [");
    bool first = true;
    for (sxmc::Signal& s : base) {
      pdfz::EvalKernel* k = dynamic_cast<pdfz::EvalKernel*>(s.histogram);
      if (!k) continue;
      sxmc::Signal shared = sxmc::share_pdfz(s);
      std::printf("%s{\"name\": \"%s\", \"signal_cutoff\": ", first ? "" : ", ", s.name.c_str());
      print_cutoff(s.bandwidth_cutoff);
      std::printf(", \"cutoff\": ");
      print_cutoff(k->Cutoff());
      std::printf(", \"shared_cutoff\": ");
      print_cutoff(static_cast<pdfz::EvalKernel*>(shared.histogram)->Cutoff());
      std::printf("}");
      delete shared.histogram;
      first = false;
    }
    std::printf("], \"events\": %zu, \"walks\": [", data.size() / (D + 1));
    sxmc::Chain chains[2];
    for (int w = 0; w < 2; w++) {
      std::vector<sxmc::Signal> signals;
      for (const sxmc::Signal& b : base) signals.push_back(sxmc::share_pdfz(b));
      try {
        sxmc::MCMC mcmc(fc.sources, signals, fc.systematics, fc.observables, 4321, nullptr);
        mcmc.reference_form = w == 0;
        chains[w] = mcmc(data, (unsigned)fc.nsteps, fc.burnin_fraction, false, 1000);
        size_t finite = 0;
        const size_t col = chains[w].names.size() - 1;
        for (size_t q = 0; q < chains[w].nrows(); q++) finite += std::isfinite(chains[w].at(q, col)) ? 1 : 0;
        std::printf("%s{\"form\": \"%s\", \"rows\": %zu, \"finite_nll_rows\": %zu, \"accepted\": %zu, \"tiles\": [",
                    w ? ", " : "", mcmc.WalkFormName(), chains[w].nrows(), finite, chains[w].accepted);
        bool f2 = true;
        for (const sxmc::Signal& s : signals) {
          pdfz::EvalKernel* k = dynamic_cast<pdfz::EvalKernel*>(s.histogram);
          if (!k) continue;
          unsigned long long visited = 0, possible = 0;
          k->CutoffStats(visited, possible);
          std::printf("%s[%llu, %llu]", f2 ? "" : ", ", visited, possible);
          f2 = false;
        }
        std::printf("]}");
      } catch (...) {
        for (sxmc::Signal& s : signals) delete s.histogram;
        throw;
      }
      for (sxmc::Signal& s : signals) delete s.histogram;
    }
    const bool same = chains[0].rows.size() == chains[1].rows.size() && chains[0].accepted == chains[1].accepted &&
                      std::memcmp(chains[0].rows.data(), chains[1].rows.data(), chains[0].rows.size() * sizeof(float)) == 0;
    std::printf("], \"same_bytes\": %s}\n", same ? "true" : "false");
    status = 0;
  } catch (const pdfz::Error& e) {
    std::printf("kde_cutoff_fit: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("kde_cutoff_fit: %s\n", e.what());
  }
  for (sxmc::Signal& s : base) delete s.histogram;
  return status;
}
