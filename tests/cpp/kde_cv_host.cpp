// kde_cv_host.cpp -- the host arithmetic of EvalKernel's bandwidth cross-validation (sxmc_amd/csrc/kde_cv.h: the grid,
// the split of a scan over workgroups, the rows a subset scores, the choice and the search) checked without a device or
// the library.  Stand-alone, so that tests/test_kde_cv_reference_cpu.py can also build and run it under ASan + UBSan.
// Exit status 0 and "kde_cv_host: ok" when every check holds.  With arguments it prints instead, for the Python
// restatement to compare with:  grid <lo> <hi> <steps> | split <m> <K> | subset <n> <max_rows>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../sxmc_amd/csrc/kde_cv.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("kde_cv_host: line %d: %s\n", __LINE__, #cond);    \
      failures++;                                                    \
    }                                                                \
  } while (0)

static int print_mode(int argc, char** argv) {
  using namespace sxkde;
  if (!std::strcmp(argv[1], "grid") && argc == 5) {
    const double lo = std::atof(argv[2]), hi = std::atof(argv[3]);
    const int steps = std::atoi(argv[4]);
    if (const char* why = cv_grid_error(lo, hi, steps)) {
      std::printf("error: %s\n", why);
      return 0;
    }
    for (double s : cv_grid(lo, hi, steps)) std::printf("%a\n", s);
    return 0;
  }
  if (!std::strcmp(argv[1], "split") && argc == 4) {
    unsigned per = 0, ns = 0;
    cv_split((size_t)std::atoll(argv[2]), std::atoi(argv[3]), per, ns);
    std::printf("%u %u\n", per, ns);
    return 0;
  }
  if (!std::strcmp(argv[1], "subset") && argc == 4) {
    for (size_t i : cv_subset((size_t)std::atoll(argv[2]), (size_t)std::atoll(argv[3]))) std::printf("%zu\n", i);
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  using namespace sxkde;
  if (argc > 1) return print_mode(argc, argv);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

  // the grid: validated; its ends are lo and hi themselves; the default has ratio 2^(1/4) and 1 on it
  CHECK(!cv_grid_error(0.125, 4.0, 21) && !cv_grid_error(1.0, 1.0, 1) && !cv_grid_error(0.5, 0.5, 32));
  CHECK(cv_grid_error(0.125, 4.0, 0) && cv_grid_error(0.125, 4.0, 33) && cv_grid_error(0.0, 4.0, 21));
  CHECK(cv_grid_error(-1.0, 4.0, 21) && cv_grid_error(4.0, 0.125, 21) && cv_grid_error(nan, 4.0, 21));
  CHECK(cv_grid_error(0.125, inf, 21) && cv_grid_error(0.125, nan, 21));
  const CvOptions def;
  const std::vector<double> g = cv_grid(def.lo, def.hi, def.steps);
  CHECK(g.size() == 21 && g.front() == 0.125 && g.back() == 4.0 && g[12] == 1.0 && g[4] == 0.25 && g[16] == 2.0);
  for (size_t k = 1; k < g.size(); k++) CHECK(std::fabs(g[k] / g[k - 1] - std::pow(2.0, 0.25)) < 1e-15);
  const std::vector<double> odd = cv_grid(0.3, 1.7, 5);
  CHECK(odd.front() == 0.3 && odd.back() == 1.7 && std::fabs(odd[2] - std::sqrt(0.3 * 1.7)) < 1e-15);
  CHECK(cv_grid(0.7, 3.0, 1).size() == 1 && cv_grid(0.7, 3.0, 1)[0] == 0.7);
  CHECK(cv_grid(2.0, 2.0, 3)[1] == 2.0);

  // the split: from m and K alone, whole grains, covers m tightly, at most kCvSplits workgroups, partials in budget
  for (int K : {1, 2, 21, 32}) {
    for (size_t m : {size_t(2), size_t(255), size_t(256), size_t(257), size_t(513), size_t(4096), size_t(4097),
                     size_t(8192), size_t(8193), size_t(65536), size_t(131072), size_t(1000003)}) {
      unsigned per = 0, ns = 0;
      cv_split(m, K, per, ns);
      CHECK(per % kCvGrain == 0 && per >= kCvGrain);
      CHECK(ns >= 1 && ns <= (unsigned)kCvSplits);
      CHECK((size_t)ns * per >= m && (size_t)(ns - 1) * per < m);
      CHECK(ns == 1 || (unsigned long long)ns * m * (unsigned long long)K <= kCvPartials + (unsigned long long)m * K);
    }
  }
  unsigned per = 0, ns = 0;
  cv_split(4096, 1, per, ns);   // the largest m that still takes the smallest per_split ...
  CHECK(per == 256 && ns == 16);
  cv_split(4097, 1, per, ns);   // ... and one past it
  CHECK(per == 512 && ns == 9);
  cv_split(256, 32, per, ns);
  CHECK(per == 256 && ns == 1);
  cv_split(257, 32, per, ns);
  CHECK(per == 256 && ns == 2);
  cv_split(8192, 32, per, ns);    // 2^22 / (8192 * 32) = 16 splits still
  CHECK(per == 512 && ns == 16);
  cv_split(8193, 32, per, ns);    // ... and 15 from here
  CHECK(per == 768 && ns == 11);
  cv_split(131072, 21, per, ns);  // the benchmark's scan: one split
  CHECK(per == 131072 && ns == 1);
  cv_split(131072, 32, per, ns);
  CHECK(ns == 1);

  // the subset: every ceil(n / max_rows)-th in-domain row from the first
  const size_t R = 100;
  for (size_t n : {R - 1, R, R + 1, 2 * R + 1}) {
    const std::vector<size_t> idx = cv_subset(n, R);
    const size_t stride = n <= R ? 1 : (n + R - 1) / R;
    CHECK(cv_stride(n, R) == stride && idx.size() == cv_subset_size(n, R) && idx.size() <= R);
    for (size_t k = 0; k < idx.size(); k++) CHECK(idx[k] == k * stride);
    CHECK(idx.back() + stride >= n);
  }
  CHECK(cv_subset(R - 1, R).size() == R - 1 && cv_subset(R, R).size() == R);
  CHECK(cv_subset(R + 1, R).size() == 51 && cv_stride(R + 1, R) == 2);       // 0, 2, ..., 100
  CHECK(cv_subset(2 * R + 1, R).size() == 67 && cv_stride(2 * R + 1, R) == 3);
  CHECK(cv_subset(1000, 0).size() == 1000 && cv_stride(1000, 0) == 1);
  CHECK(cv_subset_size(2, 1) == 1 && cv_subset_size(3, 2) == 2);

  // the choice: the largest finite score; ties to the smaller |ln s|, then the smaller s; nothing finite: -1
  CHECK(cv_choose({0.5, 1.0, 2.0}, {-3.0, -2.0, -2.5}) == 1);
  CHECK(cv_choose({0.5, 1.0, 2.0}, {-inf, nan, -2.5}) == 2);
  CHECK(cv_choose({0.25, 0.5, 2.0}, {-1.0, -1.0, -1.0}) == 1);   // |ln 0.5| = |ln 2| < |ln 0.25|; then the smaller s
  CHECK(cv_choose({0.5, 2.0}, {-1.0, -1.0}) == 0 && cv_choose({2.0, 0.5}, {-1.0, -1.0}) == 1);
  CHECK(cv_choose({0.25, 1.0, 4.0}, {-1.0, -1.0, -0.5}) == 2);
  CHECK(cv_choose({0.5, 1.0}, {-inf, -inf}) == -1 && cv_choose({0.5, 1.0}, {nan, inf}) == -1);

  // the search over a scorer with a known optimum at (0.5, 2) in ln-quadratic form: the score never decreases, the
  // coordinate scans hold the others at the values chosen so far, the report says what was chosen
  {
    CvOptions o;
    o.lo = 0.25;
    o.hi = 4.0;
    o.steps = 9;   // ratio sqrt 2: 0.5, 1 and 2 on the grid
    int calls = 0;
    const auto scorer = [&](const double* mult, int K, double* out) {
      calls++;
      for (int c = 0; c < K; c++) {
        const double a = std::log(mult[c * 2] / 0.5), b = std::log(mult[c * 2 + 1] / 2.0);
        out[c] = -(a * a) - 2.0 * (b * b);
      }
      return 0;
    };
    CvReport rep;
    std::string err;
    CHECK(cv_search(o, 2, scorer, rep, err) == 0 && calls == 3 && rep.scans.size() == 3);
    CHECK(rep.scale[0] == 0.5 && rep.scale[1] == 2.0 && rep.score == 0.0);
    CHECK(rep.has_one && std::fabs(rep.score_at_one + std::log(2.0) * std::log(2.0) * 3.0) < 1e-15);
    CHECK(rep.scans[0].observable == -1 && rep.scans[1].observable == 0 && rep.scans[2].observable == 1);
    double last = -inf;
    for (const CvScan& s : rep.scans) {
      CHECK(s.chosen >= 0 && s.scores[(size_t)s.chosen] >= last);
      last = s.scores[(size_t)s.chosen];
    }
    CHECK(rep.at_edge[0] == 0 && rep.at_edge[1] == 0);
    o.per_observable = false;
    CHECK(cv_search(o, 2, scorer, rep, err) == 0 && rep.scans.size() == 1 && rep.scale[0] == rep.scale[1]);
    // an optimum off the grid's end is reported at the edge
    o.lo = 1.0;
    o.steps = 5;
    o.per_observable = true;
    CHECK(cv_search(o, 2, scorer, rep, err) == 0 && rep.scale[0] == 1.0 && rep.at_edge[0] == 1 && rep.at_edge[1] == 0);
    // 1 not on the grid: no score there
    o.lo = 0.3;
    o.hi = 0.9;
    CHECK(cv_search(o, 2, scorer, rep, err) == 0 && !rep.has_one && rep.score_at_one != rep.score_at_one);
    // a scorer's own failure stops the search with its code; no finite score is an error with a message
    CHECK(cv_search(o, 2, [](const double*, int, double*) { return 7; }, rep, err) == 7);
    CHECK(cv_search(o, 2, [&](const double*, int K, double* out) {
            for (int c = 0; c < K; c++) out[c] = -inf;
            return 0;
          }, rep, err) == -1 && err.find("no finite score") != std::string::npos);
  }
  if (failures == 0) std::printf("kde_cv_host: ok\n");
  return failures ? 1 : 0;
}
