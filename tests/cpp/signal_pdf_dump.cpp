// signal_pdf_dump.cpp -- prints every signal's "pdf" and "bandwidth_scale" as sxmc::load_config (config.h) reads them,
// as one JSON line, or "signal_pdf_dump: <message>" on stderr and exit status 1 when the configuration is refused.
// No device call and no table is read.  Built and compared with sxmc_amd/io.py by tests/test_kde_sample_cpu.py.
// Usage: signal_pdf_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: signal_pdf_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    std::printf("{\"signals\": [");
    for (size_t i = 0; i < fc.signals.size(); i++) {
      const sxmc::Signal& s = fc.signals[i];
      std::printf("%s{\"name\": \"%s\", \"pdf\": \"%s\", \"bandwidth_scale\": [", i ? ", " : "", s.name.c_str(),
                  s.pdf.c_str());
      for (size_t k = 0; k < s.bandwidth_scale.size(); k++) std::printf("%s%.17g", k ? ", " : "", s.bandwidth_scale[k]);
      std::printf("]}");
    }
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "signal_pdf_dump: %s\n", e.what());
    return 1;
  }
}
