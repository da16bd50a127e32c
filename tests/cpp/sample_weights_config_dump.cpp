// sample_weights_config_dump.cpp -- prints what sxmc::load_config (config.h) makes of every signal's "weight_field": the
// sample fields, and per signal n_mc, nexpected, the scale's k, the rows kept and their multiplicities, as one JSON line;
// or "sample_weights_config_dump: <message>" on stderr and exit status 1 when the configuration is refused.  Reads the
// tables; no device call.  Built and compared with sxmc_amd/io.py by tests/test_sample_weights_config_cpu.py.
// Usage: sample_weights_config_dump <config.json>
#include <cstdio>

#include "../../sxmc_amd/include/sxmc/config.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: sample_weights_config_dump <config.json>\n");
    return 2;
  }
  try {
    const sxmc::FitConfig fc = sxmc::load_config(argv[1]);
    std::printf("{\"sample_fields\": [");
    for (size_t i = 0; i < fc.sample_fields.size(); i++) std::printf("%s\"%s\"", i ? ", " : "", fc.sample_fields[i].c_str());
    std::printf("], \"signals\": [");
    for (size_t i = 0; i < fc.signals.size(); i++) {
      const sxmc::Signal& s = fc.signals[i];
      std::printf("%s{\"name\": \"%s\", \"n_mc\": %zu, \"nexpected\": %.17g, \"log2_scale\": %d, \"rows\": %zu, \"multiplicities\": [",
                  i ? ", " : "", s.name.c_str(), s.n_mc, s.nexpected, s.weight_log2_scale, fc.tables[i].size() / fc.nfields);
      for (size_t k = 0; k < s.multiplicities.size(); k++) std::printf("%s%u", k ? ", " : "", s.multiplicities[k]);
      std::printf("]}");
    }
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sample_weights_config_dump: %s\n", e.what());
    return 1;
  }
}
