// constraint_config_dump.cpp -- prints the fit's "constraint_correlations" as sxmc::load_config (config.h) scatters
// them into the P x P correlation matrix, as one JSON line ({"rho": null} without the key, else {"rho": [row-major
// numbers]}), or "constraint_config_dump: <message>" on stderr and exit status 1 when the configuration is refused.
// No device call and no table is read.  Built and compared with sxmc_amd/io.py by tests/test_constraint_config_cpu.py.
// Usage: constraint_config_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: constraint_config_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    if (fc.constraint_correlation.empty()) {
      std::printf("{\"rho\": null}\n");
      return 0;
    }
    std::printf("{\"rho\": [");
    for (size_t k = 0; k < fc.constraint_correlation.size(); k++) {
      std::printf("%s%.17g", k ? ", " : "", fc.constraint_correlation[k]);
    }
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "constraint_config_dump: %s\n", e.what());
    return 1;
  }
}
