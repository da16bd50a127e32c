// test_kde_walk.cpp -- sxmc::MCMC over one kernel-density signal and one histogram signal, written with the reference's
// spelling (Signal::histogram = new pdfz::EvalKernel(...)).  A chain with a pdfz::EvalKernel walks the per-evaluator
// path (EvalAsync / EvalFinished on every evaluator, then the NLL kernels).  Prints one JSON line; exit status 0 when
// the walk took every step, its acceptance lies in (0, 1) and every recorded NLL is finite.  Without a GPU it says so
// and exits 0.  Built and run by tests/test_kde_cpu.py (no device) and tests/test_gpu_kde.py.
//
// test_kde_walk [nsteps [outdir]]: with outdir, also writes what a host recomputation of the recorded NLLs needs
// (tests/test_gpu_kde_walk.py) as raw little-endian arrays -- flat.f32 and line.f32 (the two tables, rows of F floats),
// data.f32 (the events, rows of value + data set), chain.f32 (the recorded rows: parameters, then the NLL) -- and
// index.json, which names them with their shapes and gives the parameter layout (names, means, sigmas), the
// systematics, the signals (nexpected, n_mc, source), the domain and binning, and the kernel signal's bandwidth.
#include <sxmc/pdfz.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/mcmc.h"

namespace {

void write_raw(const std::string& path, const std::vector<float>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
  if (!f) throw std::runtime_error("cannot write " + path);
}

std::string json_list(const std::vector<double>& v) {
  std::string s = "[";
  char buf[64];
  for (size_t i = 0; i < v.size(); i++) {
    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    s += buf;
  }
  return s + "]";
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned nsteps = argc > 1 ? (unsigned)std::atoi(argv[1]) : 3000u;
  const std::string outdir = argc > 2 ? argv[2] : "";
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("test_kde_walk: no GPU device, nothing to walk\n");
    return 0;
  }
  try {
    const int F = 2;   // energy, true energy
    std::vector<sxmc::Observable> observables(1);
    observables[0].name = "energy";
    observables[0].field_index = 0;
    observables[0].bins = 25;
    observables[0].lower = 0.0f;
    observables[0].upper = 10.0f;
    std::vector<sxmc::Systematic> systematics(2);
    systematics[0].name = "e_scale";
    systematics[0].type = pdfz::Systematic::SCALE;
    systematics[0].observable_field_index = 0;
    systematics[0].sigmas = {0.02};
    systematics[1].name = "e_res";
    systematics[1].type = pdfz::Systematic::RESOLUTION_SCALE;
    systematics[1].observable_field_index = 0;
    systematics[1].truth_field_index = 1;
    systematics[1].sigmas = {0.05};
    for (size_t q = 0; q < systematics.size(); q++) {
      systematics[q].means = {0.0};
      systematics[q].pidx = {(short)q};
    }

    std::mt19937_64 rng(7);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    // signal 0: a falling spectrum with many samples (histogram); signal 1: a narrow line with few (kernel density)
    std::vector<float> flat, line;
    for (int i = 0; i < 200000; i++) {
      const float t = 10.0f * uni(rng) * uni(rng);
      flat.push_back(t + 0.2f * gauss(rng));
      flat.push_back(t);
    }
    for (int i = 0; i < 3000; i++) {
      const float t = 6.0f + 0.4f * gauss(rng);
      line.push_back(t + 0.2f * gauss(rng));
      line.push_back(t);
    }
    std::vector<sxmc::Source> sources;
    std::vector<sxmc::Signal> signals(2);
    const double nexp[2] = {600.0, 300.0};
    for (int j = 0; j < 2; j++) {
      signals[j].name = j == 0 ? "spectrum" : "line";
      signals[j].source = sxmc::Source(signals[j].name, (size_t)j, 1.0f, 0.0f, false);
      signals[j].nexpected = nexp[j];
      sources.push_back(signals[j].source);
    }
    sxmc::build_pdfz(signals[0], flat, F, observables, systematics);
    pdfz::EvalKernel* kde = new pdfz::EvalKernel(line, F, 1, {0.0}, {10.0}, {1.0});
    signals[1].histogram = kde;
    signals[1].n_mc = line.size() / F;
    for (sxmc::Systematic& s : systematics) {
      auto pars = std::make_shared<pdfz::Array<short>>(s.npars, true);
      pars->writeOnlyHostPtr()[0] = s.pidx[0];
      signals[1].par_arrays.push_back(pars);
      if (s.type == pdfz::Systematic::SCALE) {
        kde->AddSystematic(pdfz::ScaleSystematic((int)s.observable_field_index, pars.get()));
      } else {
        kde->AddSystematic(pdfz::ResolutionScaleSystematic((int)s.observable_field_index, (int)s.truth_field_index,
                                                           pars.get()));
      }
    }

    // data: draws from both tables, last column the data set
    std::vector<float> data;
    for (int j = 0; j < 2; j++) {
      const std::vector<float>& tab = j == 0 ? flat : line;
      for (int e = 0; e < (int)nexp[j]; e++) {
        const size_t i = rng() % (tab.size() / F);
        const float x = tab[i * F];
        if (!(x >= 0.0f && x < 10.0f)) continue;
        data.push_back(x);
        data.push_back(0.0f);
      }
    }

    size_t rows = 0, finite = 0, accepted = 0;
    sxmc::Chain chain;
    {
      sxmc::MCMC mcmc(sources, signals, systematics, observables, 4321, nullptr);
      chain = mcmc(data, nsteps, 0.1f, false, 1000);
      rows = chain.nrows();
      accepted = chain.accepted;
      const size_t col = chain.names.size() - 1;   // "likelihood"
      for (size_t r = 0; r < rows; r++) finite += std::isfinite(chain.at(r, col)) ? 1 : 0;
    }
    std::vector<double> h = kde->Bandwidths();
    if (!outdir.empty()) {
      write_raw(outdir + "/flat.f32", flat);
      write_raw(outdir + "/line.f32", line);
      write_raw(outdir + "/data.f32", data);
      write_raw(outdir + "/chain.f32", chain.rows);
      std::vector<double> means, sigmas;
      for (const sxmc::Source& s : sources) {
        means.push_back(s.mean);
        sigmas.push_back(s.sigma);
      }
      std::string names = "[", systs = "[";
      for (const std::string& n : chain.names) names += std::string(names.size() > 1 ? ", " : "") + "\"" + n + "\"";
      for (size_t q = 0; q < systematics.size(); q++) {
        const sxmc::Systematic& s = systematics[q];
        means.insert(means.end(), s.means.begin(), s.means.end());
        sigmas.insert(sigmas.end(), s.sigmas.begin(), s.sigmas.end());
        const bool res = s.type == pdfz::Systematic::RESOLUTION_SCALE;
        systs += std::string(q ? ", " : "") + "{\"type\": \"" + (res ? "resolution_scale" : "scale") +
                 "\", \"obs\": " + std::to_string(s.observable_field_index) +
                 ", \"true_obs\": " + std::to_string(res ? s.truth_field_index : 0) +
                 ", \"pars\": [" + std::to_string(s.pidx[0]) + "]}";
      }
      std::ofstream f(outdir + "/index.json");
      f << "{\"arrays\": {\"flat\": [\"flat.f32\", " << flat.size() / F << ", " << F << "], "
        << "\"line\": [\"line.f32\", " << line.size() / F << ", " << F << "], "
        << "\"data\": [\"data.f32\", " << data.size() / 2 << ", 2], "
        << "\"chain\": [\"chain.f32\", " << rows << ", " << chain.names.size() << "]}, "
        << "\"names\": " << names << "], \"means\": " << json_list(means) << ", \"sigmas\": "
        << json_list(sigmas) << ", \"systematics\": " << systs << "], "
        << "\"nexpected\": " << json_list({signals[0].nexpected, signals[1].nexpected}) << ", "
        << "\"n_mc\": [" << signals[0].n_mc << ", " << signals[1].n_mc << "], \"source_id\": [0, 1], "
        << "\"nsources\": " << sources.size() << ", \"lower\": [0.0], \"upper\": [10.0], \"bins\": [25], "
        << "\"bandwidth_scale\": [1.0], \"bandwidth\": " << json_list(h) << ", \"nfields\": " << F << "}\n";
      if (!f) throw std::runtime_error("cannot write " + outdir + "/index.json");
    }
    for (sxmc::Signal& s : signals) delete s.histogram;
    const double acceptance = (double)accepted / nsteps;
    const bool ok = rows > 0 && finite == rows && acceptance > 0.0 && acceptance < 1.0;
    std::printf("{\"nsteps\": %u, \"accepted\": %zu, \"acceptance\": %.6f, \"rows\": %zu, \"finite_nll_rows\": %zu, "
                "\"bandwidth\": %.9g, \"ok\": %s}\n",
                nsteps, accepted, acceptance, rows, finite, h[0], ok ? "true" : "false");
    return ok ? 0 : 1;
  } catch (const pdfz::Error& e) {
    std::printf("test_kde_walk: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("test_kde_walk: %s\n", e.what());
  }
  return 1;
}
