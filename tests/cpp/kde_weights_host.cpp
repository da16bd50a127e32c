// kde_weights_host -- the bandwidth law of a pdfz::EvalKernel over weighted Monte Carlo samples
// (sxmc_amd/csrc/kde_weights.h, the code behind sxmc_kde_create_weighted and sxmc_kde_weighted_bandwidths) as a
// stand-alone host program, so that it can run under ASan + UBSan: no device, no library.
//   kde_weights_host IN OUT
// IN  (binary, native order): uint64 nrows, uint64 nfields, uint64 D, uint64 has_m, double lower[D], double upper[D],
//                             double scale[D], float table[nrows * nfields], uint32 m[nrows] (has_m only)
// OUT (binary): int64 status (sxkde::WeightedBandwidthStatus), int64 observable, uint64 live, double s1, s2, n_eff,
//               double mean[4], sigma[4], h[4]
// tests/test_kde_weighted_reference_cpu.py writes IN for each of its cases and holds OUT to
// tests/kde_weighted_reference.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sxmc_amd/csrc/kde_plan.h"
#include "../../sxmc_amd/csrc/kde_weights.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) {
    std::perror(argv[1]);
    return 2;
  }
  uint64_t head[4] = {0, 0, 0, 0};
  bool ok = std::fread(head, sizeof head, 1, in) == 1 && head[0] <= (1u << 24) && head[1] >= 1 && head[1] <= 16 &&
            head[2] >= 1 && head[2] <= (uint64_t)sxkde::kWeightsMaxDim && head[2] <= head[1] && head[3] <= 1;
  const size_t nrows = (size_t)head[0], nfields = (size_t)head[1];
  const int D = (int)head[2];
  std::vector<double> lower, upper, scale;
  std::vector<float> table;
  std::vector<unsigned> m;
  if (ok) {
    lower.resize((size_t)D);
    upper.resize((size_t)D);
    scale.resize((size_t)D);
    table.resize(nrows * nfields);
    m.resize(head[3] ? nrows : 0);
    ok = std::fread(lower.data(), sizeof(double), lower.size(), in) == lower.size() &&
         std::fread(upper.data(), sizeof(double), upper.size(), in) == upper.size() &&
         std::fread(scale.data(), sizeof(double), scale.size(), in) == scale.size() &&
         std::fread(table.data(), sizeof(float), table.size(), in) == table.size() &&
         std::fread(m.data(), sizeof(unsigned), m.size(), in) == m.size();
  }
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  const std::vector<size_t> inside = sxkde::rows_inside(table.data(), nfields, 1, nrows, D, lower.data(), upper.data());
  const sxkde::WeightedBandwidths r =
      sxkde::weighted_bandwidths(table.data(), nfields, inside, D, scale.data(), head[3] ? m.data() : nullptr);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  const int64_t codes[2] = {(int64_t)r.status, (int64_t)r.observable};
  const uint64_t live = r.live;
  const double sums[3] = {r.s1, r.s2, r.n_eff};
  ok = std::fwrite(codes, sizeof codes, 1, out) == 1 && std::fwrite(&live, sizeof live, 1, out) == 1 &&
       std::fwrite(sums, sizeof sums, 1, out) == 1 && std::fwrite(r.mean, sizeof r.mean, 1, out) == 1 &&
       std::fwrite(r.sigma, sizeof r.sigma, 1, out) == 1 && std::fwrite(r.h, sizeof r.h, 1, out) == 1;
  ok = std::fclose(out) == 0 && ok;
  return ok ? 0 : 1;
}
