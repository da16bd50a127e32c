// signal_cv_dump.cpp -- prints every signal's "pdf", whether its bandwidth scales are to be chosen by cross-validation
// ("bandwidth_scale": "cv") and the grid and search of "bandwidth_cv", as sxmc::load_config (config.h) reads them, as
// one JSON line, or "signal_cv_dump: <message>" on stderr and exit status 1 when the configuration is refused.  No
// device call and no table is read.  Built and compared with sxmc_amd/io.py by tests/test_kde_cv_config_cpu.py.
// Usage: signal_cv_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: signal_cv_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    std::printf("{\"signals\": [");
    for (size_t i = 0; i < fc.signals.size(); i++) {
      const sxmc::Signal& s = fc.signals[i];
      std::printf("%s{\"name\": \"%s\", \"pdf\": \"%s\", \"cv\": %s, \"lo\": %.17g, \"hi\": %.17g, \"steps\": %d, "
                  "\"per_observable\": %s, \"max_rows\": %zu, \"bandwidth_scale\": [", i ? ", " : "", s.name.c_str(),
                  s.pdf.c_str(), s.bandwidth_cv ? "true" : "false", s.cv.lo, s.cv.hi, s.cv.steps,
                  s.cv.per_observable ? "true" : "false", s.cv.max_rows);
      for (size_t d = 0; d < s.bandwidth_scale.size(); d++) std::printf("%s%.17g", d ? ", " : "", s.bandwidth_scale[d]);
      std::printf("]}");
    }
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "signal_cv_dump: %s\n", e.what());
    return 1;
  }
}
