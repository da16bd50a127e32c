// hist_sample_dump.cpp -- pdfz::EvalHist::SampleEvents dumped for comparison with pdfz.EvalHist.RandomSample (Python)
// and the numpy replica of the sampler (tests/hist_sample_reference.py): one evaluator over a table from a file, a
// shift systematic on observable 0, a fill (EvalAsync(false)), then the events of one seed as raw little-endian floats.
// Built by tests/cpp/Makefile, run by tests/test_gpu_hist_sample.py.  Without a GPU it says so and exits 0.
//
// hist_sample_dump table.f32 nfields lower,.. upper,.. nbins,.. shift seed nevents out.f32 [cut_lower,.. cut_upper,..]
//
// hist_sample_dump --host lower upper nbins seed nevents out.f32: no device -- the host sampler sxmc::random_sample
// (ensemble.h) over one observable whose bin i holds i % 3 counts, for tests/test_hist_sample_reference_cpu.py.
// hist_sample_dump --float lower upper nbins npoints out.f32: no device -- sxmc::sample_float of the points
// lower + (i % nbins + ((i * 2654435761 mod 2^32) + 0.5) 2^-32) width, i = 0 .. npoints - 1, for the same file.
#include <sxmc/pdfz.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/ensemble.h"

namespace {

template <typename T>
std::vector<T> list_of(const std::string& text) {
  std::vector<T> out;
  std::stringstream ss(text);
  std::string item;
  while (std::getline(ss, item, ',')) out.push_back((T)std::strtod(item.c_str(), nullptr));
  return out;
}

}  // namespace

int host_sampler(char** argv) {
  std::vector<sxmc::Observable> obs(1);
  obs[0].lower = std::strtof(argv[2], nullptr);
  obs[0].upper = std::strtof(argv[3], nullptr);
  obs[0].bins = (size_t)std::atoi(argv[4]);
  std::vector<unsigned> bins(obs[0].bins);
  for (size_t i = 0; i < bins.size(); i++) bins[i] = (unsigned)(i % 3);
  std::mt19937_64 rng(std::strtoull(argv[5], nullptr, 10));
  std::vector<float> events;
  sxmc::random_sample(rng, bins, obs, (size_t)std::strtoull(argv[6], nullptr, 10), 0, events);
  std::ofstream out(argv[7], std::ios::binary);
  out.write(reinterpret_cast<const char*>(events.data()), (std::streamsize)(events.size() * sizeof(float)));
  return out ? 0 : 1;
}

int float_step(char** argv) {
  const double lower = std::strtod(argv[2], nullptr), upper = std::strtod(argv[3], nullptr);
  const int nbins = std::atoi(argv[4]);
  const double width = (upper - lower) / nbins, scale = nbins / (upper - lower);
  const unsigned long long n = std::strtoull(argv[5], nullptr, 10);
  std::vector<float> out(n);
  for (unsigned long long i = 0; i < n; i++) {
    const size_t idx = (size_t)(i % (unsigned long long)nbins);
    const double u = ((double)((i * 2654435761ull) & 0xFFFFFFFFull) + 0.5) * 2.3283064365386963e-10;
    out[i] = sxmc::sample_float(lower + ((double)idx + u) * width, idx, lower, upper, scale);
  }
  std::ofstream f(argv[6], std::ios::binary);
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(float)));
  return f ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 8 && std::string(argv[1]) == "--host") return host_sampler(argv);
  if (argc == 7 && std::string(argv[1]) == "--float") return float_step(argv);
  if (argc != 10 && argc != 12) {
    std::fprintf(stderr, "usage: hist_sample_dump table.f32 nfields lower,.. upper,.. nbins,.. shift seed nevents "
                         "out.f32 [cut_lower,.. cut_upper,..]\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("hist_sample_dump: no GPU device, nothing to draw\n");
    return 0;
  }
  try {
    std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + argv[1]);
    std::vector<float> table((size_t)f.tellg() / sizeof(float));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(table.data()), (std::streamsize)(table.size() * sizeof(float)));
    const int nfields = std::atoi(argv[2]);
    const std::vector<double> lower = list_of<double>(argv[3]), upper = list_of<double>(argv[4]);
    const std::vector<int> nbins = list_of<int>(argv[5]);
    const unsigned long long seed = std::strtoull(argv[7], nullptr, 10);
    const size_t nevents = (size_t)std::strtoull(argv[8], nullptr, 10);

    pdfz::EvalHist ev(table, nfields, (int)nbins.size(), lower, upper, nbins);
    hemi::Array<short> pars(1, true);
    pars.writeOnlyHostPtr()[0] = 0;
    ev.AddSystematic(pdfz::ShiftSystematic(0, &pars));
    hemi::Array<double> params(1, true);
    params.writeOnlyHostPtr()[0] = std::strtod(argv[6], nullptr);
    hemi::Array<unsigned int> norm(1, true);
    norm.writeOnlyHostPtr()[0] = 0;
    ev.SetNormalizationBuffer(&norm);
    ev.SetParameterBuffer(&params);
    ev.EvalAsync(false);
    ev.EvalFinished();

    std::vector<float> events;
    if (argc == 12) {
      ev.SampleEvents(events, nevents, seed, list_of<float>(argv[11]), list_of<float>(argv[10]));
    } else {
      ev.SampleEvents(events, nevents, seed);
    }
    std::ofstream out(argv[9], std::ios::binary);
    out.write(reinterpret_cast<const char*>(events.data()), (std::streamsize)(events.size() * sizeof(float)));
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[9]);
    std::printf("hist_sample_dump: %zu events, norm %u\n", nevents, norm.readOnlyHostPtr()[0]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hist_sample_dump: %s\n", e.what());
    return 1;
  }
  return 0;
}
