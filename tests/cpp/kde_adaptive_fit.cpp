// kde_adaptive_fit.cpp -- a fit whose kernel-density signal has adaptive bandwidths ("bandwidth_sensitivity"), from a
// configuration file through the C++ layers: sxmc::load_config, build_pdfz, then
//   - the kernel signal's evaluator evaluated at the points of a file (rows of nobservables + 1 floats) with every
//     parameter at `value`: its values and its local factors written out raw, for the comparison with the Python
//     evaluator (tests/test_gpu_kde_adaptive.py: bit for bit);
//   - sxmc::ensemble_concurrent over experiments 0 and 1 with two lanes.
// Prints one JSON line: the sensitivity the evaluator reports, the norm, whether every interval of every experiment is
// finite, and the accepted steps.  Without a GPU it says so and exits 0.
// Usage: kde_adaptive_fit <config.json> <points.f32> <value> <values_out.f32> <factors_out.f64>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/config.h"
#include "../../sxmc_amd/include/sxmc/ensemble.h"

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: kde_adaptive_fit <config.json> <points.f32> <value> <values_out.f32> <factors_out.f64>\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("kde_adaptive_fit: no GPU device, nothing to run\n");
    return 0;
  }
  try {
    sxmc::FitConfig fc = sxmc::load_config(argv[1]);
    std::vector<sxmc::Signal> signals = fc.signals;
    for (size_t j = 0; j < signals.size(); j++)
      sxmc::build_pdfz(signals[j], fc.tables[j], (int)fc.nfields, fc.observables, fc.systematics);
    pdfz::EvalKernel* kernel = nullptr;
    for (sxmc::Signal& s : signals)
      if (s.pdf == "kernel") kernel = dynamic_cast<pdfz::EvalKernel*>(s.histogram);
    if (!kernel) throw std::runtime_error("the configuration has no kernel signal");

    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + argv[2]);
    std::vector<float> points((size_t)f.tellg() / sizeof(float));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(points.data()), (std::streamsize)(points.size() * sizeof(float)));
    const size_t npoints = points.size() / (fc.observables.size() + 1);
    const double value = std::strtod(argv[3], nullptr);
    pdfz::Array<double> params(16, true);
    for (size_t i = 0; i < 16; i++) params.writeOnlyHostPtr()[i] = value;
    pdfz::Array<unsigned int> norm(1, true);
    norm.writeOnlyHostPtr()[0] = 0;
    pdfz::Array<float> pdf(npoints, true);
    for (size_t i = 0; i < npoints; i++) pdf.writeOnlyHostPtr()[i] = 0.0f;
    kernel->SetEvalPoints(points);
    kernel->SetPDFValueBuffer(&pdf);
    kernel->SetNormalizationBuffer(&norm);
    kernel->SetParameterBuffer(&params);
    kernel->EvalAsync(true);
    kernel->EvalFinished();
    const std::vector<double> lambda = kernel->LocalFactors();
    {
      std::ofstream out(argv[4], std::ios::binary);
      out.write(reinterpret_cast<const char*>(pdf.readOnlyHostPtr()), (std::streamsize)(npoints * sizeof(float)));
      std::ofstream fac(argv[5], std::ios::binary);
      fac.write(reinterpret_cast<const char*>(lambda.data()), (std::streamsize)(lambda.size() * sizeof(double)));
      if (!out || !fac) throw std::runtime_error("cannot write the outputs");
    }
    const double alpha = kernel->BandwidthSensitivity();
    const unsigned n = norm.readOnlyHostPtr()[0];
    kernel->ForgetBuffers();

    const std::vector<unsigned> ks = {0, 1};
    const std::vector<sxmc::ExperimentResult> r =
        sxmc::ensemble_concurrent(ks, (unsigned long long)fc.seed, fc.sources, signals, fc.systematics, fc.observables,
                                  fc.nsteps, fc.burnin_fraction, 2);
    for (sxmc::Signal& s : signals) delete s.histogram;
    bool finite = r.size() == ks.size();
    size_t accepted = 0;
    for (const sxmc::ExperimentResult& e : r) {
      accepted += e.accepted;
      finite = finite && !e.intervals.empty();
      for (const sxmc::Interval& i : e.intervals)
        finite = finite && std::isfinite(i.point_estimate) && std::isfinite(i.lower) && std::isfinite(i.upper);
    }
    std::printf("{\"sensitivity\": %.17g, \"norm\": %u, \"nfactors\": %zu, \"experiments\": %zu, \"finite\": %s, "
                "\"accepted\": %zu}\n", alpha, n, lambda.size(), r.size(), finite ? "true" : "false", accepted);
    return finite ? 0 : 1;
  } catch (const pdfz::Error& e) {
    std::printf("kde_adaptive_fit: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("kde_adaptive_fit: %s\n", e.what());
  }
  return 1;
}
