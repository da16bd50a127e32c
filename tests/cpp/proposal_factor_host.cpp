// proposal_factor_host -- the re-tuning of a correlated proposal (sxmc_amd/csrc/proposal_factor.h, the code behind
// sxmc_proposal_factor) as a stand-alone host program, so that it can run under ASan + UBSan: no device, no library.
//   proposal_factor_host IN OUT
// IN  (binary, native order): int64 P, int64 nrows, double shrinkage, float widths[P], float rows[nrows * (P + 1)]
// OUT (binary): double shrinkage_used, double factor[P * P] in the device's layout (L_ij at [j * P + i])
// tests/test_proposal_factor_cpu.py writes IN for each of its cases and holds OUT to tests/step_reference_cov.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sxmc_amd/csrc/proposal_factor.h"

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
  int64_t P = 0, nrows = 0;
  double shrinkage = 0.0;
  bool ok = std::fread(&P, sizeof P, 1, in) == 1 && std::fread(&nrows, sizeof nrows, 1, in) == 1 &&
            std::fread(&shrinkage, sizeof shrinkage, 1, in) == 1 && P >= 1 && P <= 4096 && nrows >= 0 &&
            nrows <= (1 << 24) && shrinkage > 0.0 && shrinkage <= 1.0;
  std::vector<float> widths, rows;
  if (ok) {
    widths.resize((size_t)P);
    rows.resize((size_t)nrows * (size_t)(P + 1));
    ok = std::fread(widths.data(), sizeof(float), widths.size(), in) == widths.size() &&
         std::fread(rows.data(), sizeof(float), rows.size(), in) == rows.size();
  }
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  std::vector<double> factor((size_t)P * (size_t)P, -1.0);
  const double used = sxproposal::proposal_factor(rows.empty() ? nullptr : rows.data(), (size_t)nrows, (size_t)P,
                                                  widths.data(), shrinkage, factor.data());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  ok = std::fwrite(&used, sizeof used, 1, out) == 1 &&
       std::fwrite(factor.data(), sizeof(double), factor.size(), out) == factor.size();
  ok = std::fclose(out) == 0 && ok;
  return ok ? 0 : 1;
}
