// fit_proposal_dump.cpp -- prints the fit's "proposal" and "proposal_shrinkage" as sxmc::load_config (config.h) reads
// them, as one JSON line, or "fit_proposal_dump: <message>" on stderr and exit status 1 when the configuration is
// refused.  No device call and no table is read.  Built and compared with sxmc_amd/io.py by
// tests/test_proposal_config_cpu.py.
// Usage: fit_proposal_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: fit_proposal_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1], /*load_tables=*/false);
    std::printf("{\"proposal\": \"%s\", \"proposal_shrinkage\": %.17g}\n", fc.proposal.c_str(), fc.proposal_shrinkage);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fit_proposal_dump: %s\n", e.what());
    return 1;
  }
}
