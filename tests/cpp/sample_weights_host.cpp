// sample_weights_host -- the quantiser of Monte Carlo sample weights (sxmc_amd/csrc/sample_multiplicities.h, the code
// behind sxmc_sample_multiplicities) as a stand-alone host program, so that it can run under ASan + UBSan: no device,
// no library.
//   sample_weights_host IN OUT
// IN  (binary, native order): uint64 n, uint64 max_total, double w[n]
// OUT (binary): int64 status (0 ok, 1 max_total, 2 weight, 3 no scale, 4 zero total), int64 row, int64 log2_scale,
//               uint64 total, uint32 m[n] (status 0 only)
// tests/test_sample_weights_cpu.py writes IN for each of its cases and holds OUT to tests/sample_weights_reference.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sxmc_amd/csrc/sample_multiplicities.h"

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
  uint64_t n = 0, max_total = 0;
  bool ok = std::fread(&n, sizeof n, 1, in) == 1 && std::fread(&max_total, sizeof max_total, 1, in) == 1 && n <= (1u << 26);
  std::vector<double> w;
  if (ok) {
    w.resize((size_t)n);
    ok = std::fread(w.data(), sizeof(double), w.size(), in) == w.size();
  }
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  std::vector<unsigned> m((size_t)n, 0xDEADBEEFu);
  const sxweights::Result r = sxweights::sample_multiplicities(w.data(), (size_t)n, max_total, m.data());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  const int64_t head[3] = {(int64_t)r.status, (int64_t)r.row, (int64_t)r.log2_scale};
  const uint64_t total = r.total;
  ok = std::fwrite(head, sizeof head, 1, out) == 1 && std::fwrite(&total, sizeof total, 1, out) == 1;
  if (ok && r.status == sxweights::Status::ok) ok = std::fwrite(m.data(), sizeof(unsigned), m.size(), out) == m.size();
  ok = std::fclose(out) == 0 && ok;
  return ok ? 0 : 1;
}
