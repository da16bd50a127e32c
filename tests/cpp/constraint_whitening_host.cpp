// constraint_whitening_host -- the validation and whitening of correlated constraints
// (sxmc_amd/csrc/constraint_whitening.h, the code behind sxmc_constraint_whitening) as a stand-alone host program, so
// that it can run under ASan + UBSan: no device, no library.
//   constraint_whitening_host IN OUT
// IN  (binary, native order): int64 P, double sigmas[P], double rho[P * P] (row-major)
// OUT (binary): int64 status (0: whitened, 1: refused, 2: not positive definite), int64 pivot (-1 unless status 2),
//               double W[P * P] in the device's layout (W_ij at [j * P + i]; only for status 0), then the message's bytes
// tests/test_constraint_whitening_cpu.py writes IN for each of its cases and holds OUT to
// tests/step_reference_constraints.py.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../sxmc_amd/csrc/constraint_whitening.h"

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
  int64_t P = 0;
  bool ok = std::fread(&P, sizeof P, 1, in) == 1 && P >= 1 && P <= 4096;
  std::vector<double> sigmas, rho;
  if (ok) {
    sigmas.resize((size_t)P);
    rho.resize((size_t)P * (size_t)P);
    ok = std::fread(sigmas.data(), sizeof(double), sigmas.size(), in) == sigmas.size() &&
         std::fread(rho.data(), sizeof(double), rho.size(), in) == rho.size();
  }
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  std::vector<double> W((size_t)P * (size_t)P, -1.0);
  int64_t status = 0, pivot = -1;
  std::string message = sxconstraint::check_correlation(rho.data(), sigmas.data(), (size_t)P);
  if (!message.empty()) {
    status = 1;
  } else {
    pivot = sxconstraint::whitening(rho.data(), (size_t)P, W.data());
    if (pivot >= 0) {
      status = 2;
      message = "constraint correlation: not positive definite at parameter " + std::to_string(pivot);
    }
  }
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  ok = std::fwrite(&status, sizeof status, 1, out) == 1 && std::fwrite(&pivot, sizeof pivot, 1, out) == 1;
  if (status == 0) ok = ok && std::fwrite(W.data(), sizeof(double), W.size(), out) == W.size();
  ok = ok && std::fwrite(message.data(), 1, message.size(), out) == message.size();
  ok = std::fclose(out) == 0 && ok;
  return ok ? 0 : 1;
}
