// test_fit_spectra.cpp -- sxmc::fit_spectra + sxmc::write_fit_spectra on a fit described by files, so that the Python
// layer (sxmc_amd/ensemble.py fit_spectra, sxmc_amd/io.py write_fit_spectra) can be run on the same inputs and the
// written spectra compared value for value.  Built and run by tests/test_gpu_fit_spectra.py (not by the Makefile).
//
// test_fit_spectra <indir> <outdir>: reads <indir>/case.txt, whitespace-separated,
//   fields F
//   observables N, then per observable: name field_index bins lower upper
//   systematics N, then per systematic: name type(0 shift, 1 scale, 2 resolution_scale, 3 ctscale) field truth_field
//                                       npars pidx...
//   sources N, then per source: name
//   signals N, then per signal: name dataset source_index nexpected n_mc pdf(hist|kernel) file rows
//                               [kernel: one bandwidth scale per observable]
//   params P, then the P values
//   data file rows
// the tables as raw little-endian float32 (rows of F floats; the data rows of observables + 1), and writes the spectra
// to <outdir>.  Without a GPU it says so and exits 0.
#include <sxmc/pdfz.h>

#include <cstdio>
#include <fstream>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sxmc_amd/include/sxmc/ensemble.h"

namespace {

std::vector<float> read_raw(const std::string& path, size_t nfloats) {
  std::vector<float> v(nfloats);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(nfloats * sizeof(float)));
  if (!f && nfloats) throw std::runtime_error("cannot read " + path);
  return v;
}

void expect(std::istream& in, const std::string& word) {
  std::string w;
  in >> w;
  if (w != word) throw std::runtime_error("case.txt: expected '" + word + "', found '" + w + "'");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: test_fit_spectra <indir> <outdir>\n");
    return 2;
  }
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("test_fit_spectra: no GPU device, nothing to project\n");
    return 0;
  }
  const std::string indir = argv[1], outdir = argv[2];
  try {
    std::ifstream in(indir + "/case.txt");
    if (!in) throw std::runtime_error("cannot read " + indir + "/case.txt");
    size_t F = 0, n = 0;
    expect(in, "fields");
    in >> F;
    expect(in, "observables");
    in >> n;
    std::vector<sxmc::Observable> observables(n);
    for (sxmc::Observable& o : observables) in >> o.name >> o.field_index >> o.bins >> o.lower >> o.upper;
    expect(in, "systematics");
    in >> n;
    std::vector<sxmc::Systematic> systematics(n);
    for (sxmc::Systematic& s : systematics) {
      int type = 0;
      in >> s.name >> type >> s.observable_field_index >> s.truth_field_index >> s.npars;
      s.type = (pdfz::Systematic::Type)type;
      s.pidx.resize(s.npars);
      for (short& p : s.pidx) in >> p;
      s.means.assign(s.npars, 0.0);
      s.sigmas.assign(s.npars, 0.1);
    }
    expect(in, "sources");
    in >> n;
    std::vector<sxmc::Source> sources(n);
    for (size_t i = 0; i < n; i++) {
      in >> sources[i].name;
      sources[i].index = i;
    }
    expect(in, "signals");
    in >> n;
    std::vector<sxmc::Signal> signals(n);
    std::set<unsigned> datasets;
    for (sxmc::Signal& s : signals) {
      size_t source = 0, rows = 0;
      std::string file;
      in >> s.name >> s.dataset >> source >> s.nexpected >> s.n_mc >> s.pdf >> file >> rows;
      if (s.pdf == "kernel") {
        s.bandwidth_scale.resize(observables.size());
        for (double& b : s.bandwidth_scale) in >> b;
      }
      s.source = sources.at(source);
      datasets.insert(s.dataset);
      sxmc::build_pdfz(s, read_raw(indir + "/" + file, rows * F), (int)F, observables, systematics);
    }
    expect(in, "params");
    in >> n;
    std::vector<double> params(n);
    for (double& p : params) in >> p;
    expect(in, "data");
    std::string file;
    in >> file >> n;
    if (!in) throw std::runtime_error("case.txt: truncated");
    const std::vector<float> data = read_raw(indir + "/" + file, n * (observables.size() + 1));

    const sxmc::FitSpectra spectra =
        sxmc::fit_spectra(params, sources, signals, systematics, observables, datasets, data);
    const std::vector<std::string> paths = sxmc::write_fit_spectra(outdir, spectra);
    for (sxmc::Signal& s : signals) delete s.histogram;
    std::printf("test_fit_spectra: %zu spectra written\n", paths.size());
    return 0;
  } catch (const pdfz::Error& e) {
    std::printf("test_fit_spectra: pdfz::Error: %s\n", e.msg.c_str());
  } catch (const std::exception& e) {
    std::printf("test_fit_spectra: %s\n", e.what());
  }
  return 1;
}
