// kde_ensemble.cpp -- whole fake experiments over a configuration with a histogram signal and a kernel-density signal:
// sxmc::ensemble, sxmc::ensemble_concurrent (2 lanes) and sxmc::ensemble_multi_gpu on device 0 with default options
// (lockstep asked for: a kernel-density signal makes it run ensemble_concurrent lanes) and the HOST_STAGING exchange.
// Prints one JSON line: whether the three agree bit for bit per experiment, and the mean and standard error of every
// source parameter's best fit (1 = the generated rate).  Without a GPU it says so and exits 0.
// Built and run by tests/test_kde_sample_cpu.py (no device) and tests/test_gpu_kde_sample.py.
// Usage: kde_ensemble <config.json> [nexperiments]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/config.h"
#include "../../sxmc_amd/include/sxmc/ensemble.h"

static bool same(const sxmc::ExperimentResult& a, const sxmc::ExperimentResult& b) {
  if (a.index != b.index || a.accepted != b.accepted || a.nevents != b.nevents) return false;
  if (a.intervals.size() != b.intervals.size()) return false;
  for (size_t p = 0; p < a.intervals.size(); p++) {
    const sxmc::Interval &x = a.intervals[p], &y = b.intervals[p];
    if (std::memcmp(&x.point_estimate, &y.point_estimate, sizeof(float)) || std::memcmp(&x.lower, &y.lower, sizeof(float)) ||
        std::memcmp(&x.upper, &y.upper, sizeof(float)))
      return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: kde_ensemble <config.json> [nexperiments]\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("kde_ensemble: no GPU device, nothing to run\n");
    return 0;
  }
  try {
    sxmc::FitConfig fc = sxmc::load_config(argv[1]);
    const unsigned nexp = argc > 2 ? (unsigned)std::atoi(argv[2]) : fc.nexperiments;
    std::vector<unsigned> ks;
    for (unsigned k = 0; k < nexp; k++) ks.push_back(k);
    const unsigned long long seed = (unsigned long long)fc.seed;
    std::vector<sxmc::Signal> signals = fc.signals;
    for (size_t j = 0; j < signals.size(); j++)
      sxmc::build_pdfz(signals[j], fc.tables[j], (int)fc.nfields, fc.observables, fc.systematics);
    const std::vector<sxmc::ExperimentResult> a =
        sxmc::ensemble(ks, seed, fc.sources, signals, fc.systematics, fc.observables, fc.nsteps, fc.burnin_fraction);
    const std::vector<sxmc::ExperimentResult> b = sxmc::ensemble_concurrent(
        ks, seed, fc.sources, signals, fc.systematics, fc.observables, fc.nsteps, fc.burnin_fraction, 2);
    for (sxmc::Signal& s : signals) delete s.histogram;

    sxmc::MultiGpuOptions opt;   // defaults: lockstep sets asked for
    opt.exchange = sxmc::MultiGpuOptions::HOST_STAGING;
    std::vector<const std::vector<float>*> tables;
    for (const std::vector<float>& t : fc.tables) tables.push_back(&t);
    const sxmc::MultiGpuEnsemble mg = sxmc::ensemble_multi_gpu({0}, nexp, seed, fc.sources, fc.signals, tables,
                                                               (int)fc.nfields, fc.systematics, fc.observables,
                                                               fc.nsteps, fc.burnin_fraction, opt);
    bool concurrent_same = a.size() == b.size(), multi_same = mg.results.size() == a.size();
    for (size_t i = 0; i < a.size() && i < b.size(); i++) concurrent_same = concurrent_same && same(a[i], b[i]);
    for (size_t i = 0; i < a.size() && i < mg.results.size(); i++) multi_same = multi_same && same(a[i], mg.results[i]);

    std::printf("{\"experiments\": %u, \"steps\": %u, \"concurrent_identical\": %s, \"multi_gpu_identical\": %s, "
                "\"device_mode\": \"%s\", \"lockstep_chains\": %u, \"sources\": {",
                nexp, fc.nsteps, concurrent_same ? "true" : "false", multi_same ? "true" : "false",
                mg.device_mode.c_str(), opt.lockstep_chains);
    for (size_t p = 0; p < fc.sources.size(); p++) {
      double sum = 0, ss = 0;
      for (const sxmc::ExperimentResult& r : a) sum += r.intervals.at(p).point_estimate;
      const double mean = sum / a.size();
      for (const sxmc::ExperimentResult& r : a) ss += std::pow(r.intervals.at(p).point_estimate - mean, 2);
      const double se = a.size() > 1 ? std::sqrt(ss / (a.size() - 1) / a.size()) : 0.0;
      std::printf("%s\"%s\": {\"mean\": %.9g, \"stderr\": %.9g}", p ? ", " : "", fc.sources[p].name.c_str(), mean, se);
    }
    size_t events = 0;
    for (const sxmc::ExperimentResult& r : a) events += r.nevents;
    std::printf("}, \"mean_events\": %.3f}\n", (double)events / a.size());
    return concurrent_same && multi_same ? 0 : 1;
  } catch (const pdfz::Error& e) {
    std::printf("kde_ensemble: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("kde_ensemble: %s\n", e.what());
  }
  return 1;
}
