// walk_dump.cpp -- whole walks of sxmc::MCMC over the small fit (small_fit.h), pinned: one line per case with the
// case's name, the chain's rows and accepted steps, a 64-bit FNV-1a hash of the bytes of Chain::rows and the first and
// last row as float bits; for the ensemble cases, per experiment the accepted steps and every interval as float bits; for
// the multi-GPU cases also a hash of the gathered block, the medians as float bits and how the devices ran.
// Every chain walks with optimize = false where the walk is built here: the trial launches time the device, and a pinned
// chain must not depend on timing.  Built by tests/cpp/Makefile, run by tests/test_gpu_walk_golden.py, which compares
// the lines with tests/golden/walk_chains.json.  Without a GPU it says so and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "small_fit.h"

namespace {

std::string bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  char buf[16];
  std::snprintf(buf, sizeof buf, "%08x", u);
  return buf;
}

std::string describe(const sxmc::Chain& c) {
  uint64_t h = 1469598103934665603ull;   // FNV-1a, 64 bit
  const unsigned char* p = reinterpret_cast<const unsigned char*>(c.rows.data());
  for (size_t i = 0; i < c.rows.size() * sizeof(float); i++) h = (h ^ p[i]) * 1099511628211ull;
  char buf[96];
  std::snprintf(buf, sizeof buf, "nrows %zu accepted %zu fnv1a %016llx", c.nrows(), c.accepted, (unsigned long long)h);
  std::string out = buf;
  const size_t ncol = c.names.size();
  for (const char* which : {"first", "last"}) {
    out += std::string(" ") + which;
    if (c.nrows() == 0) continue;
    const size_t row = which[0] == 'f' ? 0 : c.nrows() - 1;
    for (size_t k = 0; k < ncol; k++) out += " " + bits(c.at(row, k));
  }
  return out;
}

std::string describe(const std::vector<sxmc::ExperimentResult>& res) {
  std::string out;
  for (const sxmc::ExperimentResult& r : res) {
    out += (out.empty() ? "experiment " : " experiment ") + std::to_string(r.index) + " accepted " +
           std::to_string(r.accepted);
    for (const sxmc::Interval& iv : r.intervals) {
      out += " [" + bits(iv.point_estimate) + " " + bits(iv.lower) + " " + bits(iv.upper) + " " + bits(iv.cl) + " " +
             bits(iv.coverage) + (iv.one_sided ? " one-sided]" : " two-sided]");
    }
  }
  return out;
}

std::string describe(const sxmc::MultiGpuEnsemble& mg) {
  uint64_t h = 1469598103934665603ull;   // FNV-1a, 64 bit
  const unsigned char* p = reinterpret_cast<const unsigned char*>(mg.gathered.data());
  for (size_t i = 0; i < mg.gathered.size() * sizeof(float); i++) h = (h ^ p[i]) * 1099511628211ull;
  char buf[48];
  std::snprintf(buf, sizeof buf, " gathered fnv1a %016llx", (unsigned long long)h);
  std::string out = describe(mg.results) + buf + " median_upper";
  for (float m : mg.median_upper) out += " " + bits(m);
  return out + " mode " + mg.device_mode;
}

void line(const std::string& name, const std::string& text) { std::printf("%s\t%s\n", name.c_str(), text.c_str()); }

}  // namespace

int main() {
  int ndev = 0;
  if (sxmc_device_count(&ndev) != SXMC_OK || ndev < 1) {
    std::printf("walk_dump: no GPU device, nothing to walk\n");
    return 0;
  }
  SmallFit fit;
  try {
    fit.SetUp();
    // seed 7, 333 steps, burn-in fraction 0.2, sync_interval 100 unless the case says otherwise
    auto walk = [&](const std::string& name, const std::function<void(sxmc::MCMC&)>& settings, bool passes = false,
                    unsigned nsteps = 333, float burnin = 0.2f, bool debug = false, unsigned sync = 100,
                    sxmc_stream_t stream = nullptr) {
      sxmc::MCMC m(fit.sources, fit.signals, fit.systematics, fit.observables, 7, stream);
      m.optimize = false;
      settings(m);
      const sxmc::Chain c = m(fit.data, nsteps, burnin, debug, sync);
      line(name, describe(c) + (passes ? std::string(" passes<333 ") + (m.LookaheadPasses() < 333 ? "1" : "0") : ""));
    };
    walk("default", [](sxmc::MCMC&) {});
    walk("graph_steps 8", [](sxmc::MCMC& m) { m.graph_steps = 8; });
    walk("lookahead, graph_steps 0", [](sxmc::MCMC& m) { m.lookahead = true; }, true);
    walk("lookahead, graph_steps 6", [](sxmc::MCMC& m) { m.lookahead = true; m.graph_steps = 6; }, true);
    walk("consume off", [](sxmc::MCMC& m) { m.consume = false; });
    walk("reference_form", [](sxmc::MCMC& m) { m.reference_form = true; });
    walk("lut_output", [](sxmc::MCMC& m) { m.lut_output = true; });
    walk("debug_mode, 40 steps, no burn-in, sync_interval 16", [](sxmc::MCMC&) {}, false, 40, 0.0f, true, 16);
    {
      // a stream of the caller's, as a lane of ensemble_concurrent sets one up: the walk does not own it
      sxmc_stream_t strm = nullptr;
      sxmc::check(sxmc_stream_create_nonblocking(&strm));
      sxmc::transfer_stream() = strm;
      std::vector<sxmc::Signal> mine;
      for (const sxmc::Signal& s : fit.signals) mine.push_back(sxmc::share_pdfz(s));
      {
        sxmc::MCMC m(fit.sources, mine, fit.systematics, fit.observables, 7, strm);
        m.optimize = false;
        m.graph_steps = 8;
        line("caller's non-blocking stream, graph_steps 8", describe(m(fit.data, 333, 0.2f, false, 100)));
      }
      for (sxmc::Signal& s : mine) delete s.histogram;
      sxmc::transfer_stream() = nullptr;
      sxmc::check(sxmc_stream_destroy(strm));
    }
    {
      const std::vector<unsigned> ks = {0u, 1u, 2u, 3u};
      const std::string seq = describe(sxmc::ensemble(ks, 31, fit.sources, fit.signals, fit.systematics,
                                                      fit.observables, 120, 0.2f, 0.9f, 100));
      const std::string lock = describe(sxmc::ensemble_lockstep(ks, 31, fit.sources, fit.signals, fit.systematics,
                                                                fit.observables, 120, 0.2f, 2, 1, 0.9f, 100, 8));
      const std::string conc = describe(sxmc::ensemble_concurrent(ks, 31, fit.sources, fit.signals, fit.systematics,
                                                                  fit.observables, 120, 0.2f, 2, 0.9f, 100, 8));
      line("ensemble_lockstep, 2 chains in 1 set, graph_steps 8", lock + (lock == seq ? " =ensemble 1" : " =ensemble 0"));
      line("ensemble_concurrent, 2 lanes, graph_steps 8", conc + (conc == seq ? " =ensemble 1" : " =ensemble 0"));
      const std::string pseq = describe(sxmc::ensemble(ks, 31, fit.sources, fit.signals, fit.systematics, fit.observables,
                                                       120, 0.2f, 0.9f, 100, 0, sxmc::ERROR_PROJECTION));
      const std::string pconc = describe(sxmc::ensemble_concurrent(ks, 31, fit.sources, fit.signals, fit.systematics,
                                                                   fit.observables, 120, 0.2f, 2, 0.9f, 100, 8, -1, nullptr,
                                                                   sxmc::ERROR_PROJECTION));
      line("ensemble_concurrent, projection intervals, 2 lanes, graph_steps 8",
           pconc + (pconc == pseq ? " =ensemble 1" : " =ensemble 0"));
    }
    {
      // two logical ranks on card 0, the host standing in for the all-gather: rank 0 runs experiments 0, 2, 4 and rank 1
      // runs 1, 3
      const std::string seq = describe(sxmc::ensemble({0u, 1u, 2u, 3u, 4u}, 31, fit.sources, fit.signals, fit.systematics,
                                                      fit.observables, 120, 0.2f, 0.9f, 100));
      std::vector<const std::vector<float>*> tabs;
      for (const std::vector<float>& t : fit.tables) tabs.push_back(&t);
      auto multi = [&](const std::string& name, unsigned lockstep_chains) {
        sxmc::MultiGpuOptions opt;
        opt.sync_interval = 100;
        opt.graph_steps = 8;
        opt.lockstep_chains = lockstep_chains;
        opt.lockstep_sets = 1;
        opt.nconcurrent = 2;
        opt.exchange = sxmc::MultiGpuOptions::HOST_STAGING;
        const sxmc::MultiGpuEnsemble mg = sxmc::ensemble_multi_gpu({0, 0}, 5, 31, fit.sources, fit.signals, tabs, 4,
                                                                   fit.systematics, fit.observables, 120, 0.2f, opt);
        line(name, describe(mg) + (describe(mg.results) == seq ? " =ensemble 1" : " =ensemble 0"));
      };
      multi("ensemble_multi_gpu, host staging, 2 ranks on device 0, lockstep 2x1", 2);
      multi("ensemble_multi_gpu, host staging, 2 ranks on device 0, concurrent 2", 0);
    }
  } catch (const pdfz::Error& e) {
    std::fprintf(stderr, "walk_dump: %s\n", e.msg.c_str());
    fit.TearDown();
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "walk_dump: %s\n", e.what());
    fit.TearDown();
    return 1;
  }
  fit.TearDown();
  return 0;
}
