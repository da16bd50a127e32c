// test_kde_plan.cpp -- the pure parts of pdfz::EvalKernel's evaluation plan (sxmc_amd/csrc/kde_plan.h: the pair sum's
// split, the projection's split, the in-domain rows of a table and the truncation mass) checked without a device or
// the library.  Stand-alone, so that tests/test_kde_plan_cpu.py can also build and run it under ASan + UBSan.
// Exit status 0 and "test_kde_plan: ok" when every check holds.
#include <cstdio>
#include <limits>

#include "../../sxmc_amd/csrc/kde_plan.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("test_kde_plan: line %d: %s\n", __LINE__, #cond);   \
      failures++;                                                     \
    }                                                                 \
  } while (0)

using namespace sxkde;

// rounds of `slots` resident workgroups times tiles per workgroup: what pair_split minimises
static unsigned long long split_cost(unsigned long long pblocks, unsigned long long slots, unsigned long long used,
                                     unsigned long long tps) {
  return (pblocks * used + slots - 1) / slots * tps;
}

int main() {
  // ---- pair_split against values pinned from the arithmetic it had as sxmc_kde.cpp's choose_split
  {
    const struct { size_t pitch, ntiles; int cus, nsplit; unsigned tps; } pinned[] = {
        {256, 1, 256, 1, 1},        {256, 512, 256, 512, 1},   {100096, 512, 256, 256, 2},
        {256, 3907, 256, 1954, 2},  {3072, 118, 256, 118, 1},  {524288, 512, 256, 1, 512},
        {524544, 512, 256, 57, 9},  {256, 512, 1, 8, 64},      {1024, 7, 304, 7, 1},
    };
    for (const auto& c : pinned) {
      int nsplit = -1;
      unsigned tps = 0;
      pair_split(c.pitch, c.ntiles, c.cus, nsplit, tps);
      CHECK(nsplit == c.nsplit && tps == c.tps);
    }
  }

  // ---- pair_split's invariants: the splits cover the tiles tightly, and no split of the same form -- t tiles to each
  // of ceil(ntiles / t) workgroups, within the cap on splits -- is cheaper, nor as cheap with fewer splits
  {
    size_t shapes = 0;
    for (size_t pitch : {256u, 768u, 3072u, 40192u, 100096u, 524288u, 524544u}) {
      for (size_t ntiles : {1u, 2u, 3u, 7u, 12u, 16u, 118u, 512u, 3907u}) {
        for (int cus : {1, 64, 256, 304}) {
          int nsplit = -1;
          unsigned tps = 0;
          pair_split(pitch, ntiles, cus, nsplit, tps);
          CHECK(nsplit >= 1 && tps >= 1);
          CHECK((unsigned long long)nsplit * tps >= ntiles && (unsigned long long)(nsplit - 1) * tps < ntiles);
          const unsigned long long pblocks = pitch / 256, slots = (unsigned long long)cus * 8;
          const unsigned long long smax = std::min<unsigned long long>(ntiles, std::max<unsigned long long>(1, 64 * slots / pblocks));
          CHECK((unsigned long long)nsplit <= smax);
          const unsigned long long cost = split_cost(pblocks, slots, (unsigned long long)nsplit, tps);
          for (unsigned long long t = 1; t <= ntiles; t++) {
            const unsigned long long used = (ntiles + t - 1) / t;
            if (used > smax) continue;
            const unsigned long long other = split_cost(pblocks, slots, used, t);
            CHECK(other >= cost);
            if (other == cost) CHECK(used >= (unsigned long long)nsplit);
          }
          shapes++;
        }
      }
    }
    std::printf("test_kde_plan: %zu shapes searched\n", shapes);
  }

  // ---- rows_inside: a row-major and a column-major view of one table give the same rows, lower in, upper out, NaN and
  // the infinities out
  {
    const double lower[2] = {-1.0, 0.5}, upper[2] = {3.0, 2.0};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float below3 = std::nextafter(3.0f, 0.0f), below_m1 = std::nextafter(-1.0f, -2.0f);
    const size_t n = 11, nfields = 3;   // (the third field is no observable: whatever it holds)
    const float table[n * nfields] = {
        -1.0f, 0.5f, nan,      // on both lower edges: in
        3.0f, 1.0f, 0.0f,      // on an upper edge: out
        0.0f, 2.0f, 0.0f,      // on the other upper edge: out
        nan, 1.0f, 0.0f,       // NaN: out
        0.0f, nan, 0.0f,       //
        inf, 1.0f, 0.0f,       // the infinities: out
        0.0f, -inf, 0.0f,      //
        1.0f, 1.0f, inf,       // inside: in
        below3, 0.5f, 0.0f,    // the last float below upper: in
        below_m1, 1.0f, 0.0f,  // the first float below lower: out
        2.5f, 1.9f, 0.0f,      // inside: in
    };
    const std::vector<size_t> want = {0, 7, 8, 10};
    CHECK(rows_inside(table, nfields, 1, n, 2, lower, upper) == want);
    float cols[2 * n];
    for (size_t i = 0; i < n; i++) {
      for (size_t d = 0; d < 2; d++) cols[d * n + i] = table[i * nfields + d];
    }
    CHECK(rows_inside(cols, 1, n, n, 2, lower, upper) == want);
    CHECK(rows_inside(table, nfields, 1, n, 1, lower, upper) == (std::vector<size_t>{0, 2, 4, 6, 7, 8, 10}));   // D = 1
    CHECK(rows_inside(table, nfields, 1, 0, 2, lower, upper).empty());
  }

  // ---- the projection's split: whole tiles to a split, at most 1024 splits that cover the rows, bins in whole waves
  for (unsigned long long npad : {256ull, 768ull, 262144ull, 262400ull}) {
    for (unsigned long long nbins : {1ull, 64ull, 65ull, 1000ull}) {
      unsigned rows_per_split = 0, nsplit = 0;
      unsigned long long pitch = 0;
      project_split(npad, nbins, rows_per_split, nsplit, pitch);
      CHECK(rows_per_split >= kPlanTile && rows_per_split % kPlanTile == 0);
      CHECK(nsplit >= 1 && nsplit <= 1024);
      CHECK((unsigned long long)nsplit * rows_per_split >= npad && (unsigned long long)(nsplit - 1) * rows_per_split < npad);
      CHECK(pitch >= nbins && pitch % kPlanProjLanes == 0 && pitch - nbins < kPlanProjLanes);
    }
  }
  {
    unsigned rows_per_split = 0, nsplit = 0;
    unsigned long long pitch = 0;
    project_split(262400, 65, rows_per_split, nsplit, pitch);   // one tile over 1024: two tiles to a split
    CHECK(rows_per_split == 512 && nsplit == 513 && pitch == 128);
    project_split(262144, 64, rows_per_split, nsplit, pitch);
    CHECK(rows_per_split == 256 && nsplit == 1024 && pitch == 64);
  }

  // ---- the truncation mass: the expression the kernels and the host typed out, operation for operation
  for (double x : {-1.0, -0.25, 0.0, 1.5, 3.0}) {
    for (double h : {0.01, 0.3, 2.0, 50.0}) {
      const double lo = -1.0, hi = 3.0, r = 1.0 / (h * 1.41421356237309504880);
      const double m = truncation_mass(x, lo, hi, r);
      CHECK(m == 0.5 * (std::erfc((x - hi) * r) - std::erfc((x - lo) * r)));
      CHECK(m > 0.0 && m <= 1.0);
    }
  }
  CHECK(truncation_mass(1.0, -1.0, 3.0, 1.0 / (0.01 * 1.41421356237309504880)) == 1.0);   // far from both edges
  CHECK(std::fabs(truncation_mass(-1.0, -1.0, 3.0, 1.0 / (0.01 * 1.41421356237309504880)) - 0.5) < 1e-15);   // on an edge

  if (failures) return 1;
  std::printf("test_kde_plan: ok\n");
  return 0;
}
