// weighted_classes_host.cpp -- no device, no library: sxplan::event_classes + sxplan::class_weights (sxmc_plan.h, what
// ensure_event_classes uploads for a group with event weights) on case files, for tests/test_weighted_classes_cpu.py,
// which holds the output to tests/weighted_events_reference.py bit for bit.  Built plain and under ASan + UBSan
// (weighted.mk).
//
//   weighted_classes_host FILE
// FILE: "S E", then S lines of E event bins, then one line of E weights as 16 hex digits each (the doubles' bit
// patterns: nothing is rounded on the way in or out).  Prints "K", then per class its members' bins, its count and its
// weight sum as 16 hex digits; then "bad <index>" for the first weight that is not a finite double >= 0, or "bad -1".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sxmc_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  size_t S = 0, E = 0;
  if (std::fscanf(f, "%zu %zu", &S, &E) != 2) return 2;
  std::vector<std::vector<int>> tables(S, std::vector<int>(E));
  for (size_t j = 0; j < S; j++)
    for (size_t i = 0; i < E; i++)
      if (std::fscanf(f, "%d", &tables[j][i]) != 1) return 2;
  std::vector<double> w(E);
  for (size_t i = 0; i < E; i++) {
    unsigned long long bits = 0;
    if (std::fscanf(f, "%llx", &bits) != 1) return 2;
    const std::uint64_t b = bits;
    std::memcpy(&w[i], &b, sizeof b);
  }
  std::fclose(f);
  std::vector<const std::vector<int>*> arr(S);
  for (size_t j = 0; j < S; j++) arr[j] = &tables[j];
  sxplan::EventClasses cls;
  sxplan::event_classes(arr, E, cls);
  std::vector<double> W;
  sxplan::class_weights(arr, E, cls, w.data(), W);
  std::printf("%zu\n", cls.K);
  for (size_t k = 0; k < cls.K; k++) {
    for (size_t j = 0; j < S; j++) std::printf("%d ", cls.tables[j * cls.K + k]);
    std::uint64_t b;
    std::memcpy(&b, &W[k], sizeof b);
    std::printf("%u %016llx\n", cls.weight[k], (unsigned long long)b);
  }
  std::printf("bad %lld\n", sxplan::first_bad_event_weight(w.data(), E));
  return 0;
}
