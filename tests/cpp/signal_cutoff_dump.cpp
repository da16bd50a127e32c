// signal_cutoff_dump.cpp -- prints every signal's "pdf" and "bandwidth_cutoff" as sxmc::load_config (config.h) reads
// them, as one JSON line (an infinite cutoff as the string "inf"), or "signal_cutoff_dump: <message>" on stderr and
// exit status 1 when the configuration is refused.  No device call and no table is read.  Built and compared with
// sxmc_amd/io.py by tests/test_kde_cutoff_config_cpu.py.
// Usage: signal_cutoff_dump <config.json>
#include <cmath>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: signal_cutoff_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    std::printf("{\"signals\": [");
    for (size_t i = 0; i < fc.signals.size(); i++) {
      const sxmc::Signal& s = fc.signals[i];
      std::printf("%s{\"name\": \"%s\", \"pdf\": \"%s\", \"bandwidth_cutoff\": ", i ? ", " : "", s.name.c_str(),
                  s.pdf.c_str());
      if (std::isinf(s.bandwidth_cutoff)) std::printf("\"inf\"}");
      else std::printf("%.17g}", s.bandwidth_cutoff);
    }
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "signal_cutoff_dump: %s\n", e.what());
    return 1;
  }
}
