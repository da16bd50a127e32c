// asimov_config_dump.cpp -- prints the fit's "asimov" as sxmc::load_config (config.h) reads it, as one JSON line, or
// "asimov_config_dump: <message>" on stderr and exit status 1 when the configuration is refused.  No device call and no
// table is read.  Built and compared with sxmc_amd/io.py by tests/test_asimov_cpu.py.
// Usage: asimov_config_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"
#include "../../sxmc_amd/include/sxmc/fake_data.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: asimov_config_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    std::printf("{\"asimov\": %s, \"nexperiments\": %d}\n", fc.asimov ? "true" : "false", (int)fc.nexperiments);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "asimov_config_dump: %s\n", e.what());
    return 1;
  }
}
