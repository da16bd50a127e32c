// kde_cv_fit.cpp -- a fit whose kernel-density signals may take their bandwidth scales from cross-validation
// ("bandwidth_scale": "cv"), from a configuration file through the C++ layers: sxmc::load_config, build_pdfz, then
// sxmc::ensemble_concurrent over experiment 0 (a mixed walk when the fit also has histogram signals).
// Prints one JSON line: per kernel signal its name, the bandwidth scales the signal carries after build_pdfz, those its
// evaluator reports, its bandwidths and whether a search made it; then the experiment's accepted steps, events and every
// interval.  Two configurations that build the same evaluators print the same "walk".  Without a GPU it says so and
// exits 0.
// Usage: kde_cv_fit <config.json>
#include <cstdio>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/config.h"
#include "../../sxmc_amd/include/sxmc/ensemble.h"

static void print_list(const char* key, const std::vector<double>& v) {
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: kde_cv_fit <config.json>\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("kde_cv_fit: no GPU device, nothing to run\n");
    return 0;
  }
  try {
    sxmc::FitConfig fc = sxmc::load_config(argv[1]);
    std::vector<sxmc::Signal> signals = fc.signals;
    for (size_t j = 0; j < signals.size(); j++)
      sxmc::build_pdfz(signals[j], fc.tables[j], (int)fc.nfields, fc.observables, fc.systematics);
    std::printf("{\"kernels\": [");
    bool first = true;
    for (sxmc::Signal& s : signals) {
      pdfz::EvalKernel* k = dynamic_cast<pdfz::EvalKernel*>(s.histogram);
      if (!k) continue;
      std::printf("%s{\"name\": \"%s\", \"pending\": %s, \"searched\": %s, \"rows_used\": %zu, ", first ? "" : ", ",
                  s.name.c_str(), s.bandwidth_cv ? "true" : "false", k->CrossValidatedScales() ? "true" : "false",
                  k->CvReport().rows_used);
      print_list("signal_scale", s.bandwidth_scale);
      std::printf(", ");
      print_list("scale", k->BandwidthScale());
      std::printf(", ");
      print_list("bandwidths", k->Bandwidths());
      std::printf("}");
      first = false;
    }
    const std::vector<unsigned> ks = {0};
    const std::vector<sxmc::ExperimentResult> r =
        sxmc::ensemble_concurrent(ks, (unsigned long long)fc.seed, fc.sources, signals, fc.systematics, fc.observables,
                                  fc.nsteps, fc.burnin_fraction, 1);
    for (sxmc::Signal& s : signals) delete s.histogram;
    std::printf("], \"walk\": {\"accepted\": %zu, \"nevents\": %zu, \"intervals\": [", r.at(0).accepted, r.at(0).nevents);
    for (size_t i = 0; i < r[0].intervals.size(); i++) {
      const sxmc::Interval& v = r[0].intervals[i];
      std::printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", (double)v.point_estimate, (double)v.lower, (double)v.upper);
    }
    std::printf("]}}\n");
    return 0;
  } catch (const pdfz::Error& e) {
    std::printf("kde_cv_fit: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("kde_cv_fit: %s\n", e.what());
  }
  return 1;
}
