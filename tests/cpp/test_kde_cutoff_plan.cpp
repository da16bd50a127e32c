// test_kde_cutoff_plan.cpp -- the pure parts of pdfz::EvalKernel's cutoff radius (sxmc_amd/csrc/kde_cutoff.h: the
// accepted R and qcut, the spatial order, the boxes and the visit test) checked without a device or the library.
// Stand-alone, so that tests/test_kde_cutoff_plan_cpu.py can also build and run it under ASan + UBSan.
// Exit status 0 and "test_kde_cutoff_plan: ok" when every check holds.
#include <cstdio>
#include <limits>
#include <random>
#include <set>

#include "../../sxmc_amd/csrc/kde_cutoff.h"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("test_kde_cutoff_plan: line %d: %s\n", __LINE__, #cond);   \
      failures++;                                                            \
    }                                                                        \
  } while (0)

using namespace sxkde;

// the pair kernels' q' of one pair, in f32: the square of the first difference, a fused multiply-add per further
// observable, times g
static float pair_q(int D, const float* p, const float* r, float g) {
  const float a0 = p[0] - r[0];
  float q = a0 * a0;
  for (int k = 1; k < D; k++) {
    const float ak = p[k] - r[k];
    q = __builtin_fmaf(ak, ak, q);
  }
  return g * q;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const float finf = std::numeric_limits<float>::infinity();

  // ---- the accepted R and qcut
  CHECK(valid_cutoff(0.0) && valid_cutoff(1.0) && valid_cutoff(3.0) && valid_cutoff(1e30) && valid_cutoff(inf));
  CHECK(!valid_cutoff(nan) && !valid_cutoff(-1.0) && !valid_cutoff(0.5) && !valid_cutoff(0.999999) && !valid_cutoff(-inf));
  CHECK(!valid_cutoff(-0.5) && valid_cutoff(-0.0));
  for (double R : {1.0, 3.0, 4.0, 6.0, 15.0, 1234.5}) {
    const double exact = R * R * 0.72134752044448170;
    const float q = cutoff_qcut(R);
    CHECK((double)q >= exact && (double)std::nextafter(q, 0.0f) < exact);   // rounded up, by less than one ulp
  }
  CHECK(cutoff_qcut(15.0) > 149.0f);
  CHECK(cutoff_qcut(inf) == finf && cutoff_qcut(1e30) == finf);

  // ---- the order: a permutation, stable, spatial
  std::mt19937 rng(12345);
  for (int D = 1; D <= 4; D++) {
    const double lower[4] = {-1.0, 0.0, 2.0, -3.0}, upper[4] = {3.0, 1.5, 8.0, -0.5};
    const size_t n = 1000, npad = 1024;
    std::vector<float> x(n * (size_t)D);
    std::uniform_real_distribution<double> u(-0.2, 1.2);   // some rows outside the domain: clamped
    for (size_t i = 0; i < n; i++) {
      for (int d = 0; d < D; d++) x[i * D + d] = (float)(lower[d] + u(rng) * (upper[d] - lower[d]));
    }
    for (size_t i = 0; i < 50; i++) {   // exact duplicates of row 7 and a NaN row: ties
      for (int d = 0; d < D; d++) x[(100 + 3 * i) * D + d] = x[7 * D + d];
    }
    x[500 * D] = std::numeric_limits<float>::quiet_NaN();
    const std::vector<uint32_t> order = cutoff_sample_order(D, x.data(), (size_t)D, n, npad, lower, upper);
    CHECK(order.size() == npad);
    std::set<uint32_t> seen(order.begin(), order.end());
    CHECK(seen.size() == npad && *seen.rbegin() == npad - 1);                 // a permutation of [0, npad)
    for (size_t k = n; k < npad; k++) CHECK(order[k] == (uint32_t)k);        // the padding stays last
    std::vector<uint32_t> keys(n);
    for (size_t i = 0; i < n; i++) {
      double v[4];
      for (int d = 0; d < D; d++) v[d] = x[i * D + d];
      keys[i] = cutoff_key(D, v, lower, upper);
    }
    for (size_t k = 1; k < n; k++) {
      const uint32_t a = order[k - 1], b = order[k];
      CHECK(keys[a] < keys[b] || (keys[a] == keys[b] && a < b));             // sorted; ties by table index
    }
    CHECK(cutoff_sample_order(D, x.data(), (size_t)D, n, npad, lower, upper) == order);   // deterministic
    if (D == 1) {   // a plain sort of the clamped coordinate
      for (size_t k = 1; k < n; k++) {
        auto clamp = [&](float v) { return !(v >= lower[0]) ? (float)lower[0] : (v > upper[0] ? (float)upper[0] : v); };
        CHECK(clamp(x[order[k - 1]]) <= clamp(x[order[k]]));
      }
    }
    // clamping: a point beyond an edge shares the key of the edge
    double out[4], edge[4];
    for (int d = 0; d < D; d++) {
      out[d] = upper[d] + 5.0;
      edge[d] = upper[d];
    }
    CHECK(cutoff_key(D, out, lower, upper) == cutoff_key(D, edge, lower, upper));
    // the points' order: live ones sorted, the others after them in their own order
    std::vector<float> pts(300 * (size_t)(D + 1), 0.0f);
    std::vector<int> codes(300, 0);
    for (size_t i = 0; i < 300; i++) {
      for (int d = 0; d < D; d++) pts[i * (D + 1) + d] = x[i * D + d];
      if (i % 7 == 3) codes[i] = -1;
      if (i % 11 == 5) codes[i] = -2;
    }
    size_t nlive = 0;
    const std::vector<uint32_t> po = cutoff_point_order(D, pts.data(), 300, codes.data(), lower, upper, &nlive);
    std::set<uint32_t> pseen(po.begin(), po.end());
    CHECK(po.size() == 300 && pseen.size() == 300);
    for (size_t k = 0; k < 300; k++) CHECK((codes[po[k]] == 0) == (k < nlive));
    for (size_t k = nlive + 1; k < 300; k++) CHECK(po[k - 1] < po[k]);
    for (size_t k = 1; k < nlive; k++) CHECK(keys[po[k - 1]] < keys[po[k]] || (keys[po[k - 1]] == keys[po[k]] && po[k - 1] < po[k]));
    size_t none = 7;
    CHECK(cutoff_point_order(D, pts.data(), 0, codes.data(), lower, upper, &none).empty() && none == 0);
  }

  // ---- boxes of constructed tiles
  {
    // fixed, D = 2: rows (c0, c1, w); the row with weight 0 does not count
    const float rows[] = {1.0f, 5.0f, 2.0f, 3.0f, -1.0f, 1.0f, 100.0f, 100.0f, 0.0f, 2.0f, 7.0f, 0.5f};
    float box[kCutBox];
    cutoff_tile_box(2, false, rows, 4, box);
    CHECK(box[0] == 1.0f && box[4] == 3.0f && box[1] == -1.0f && box[5] == 7.0f && box[8] == 1.0f);
    CHECK(box[2] == finf && box[6] == -finf);   // the observables the evaluator does not have
    // adaptive, D = 1: rows (c, g, W); the smallest g among the live rows
    const float arows[] = {4.0f, 0.25f, 1.0f, 2.0f, 100.0f, 1.0f, 9.0f, 0.01f, 0.0f};
    cutoff_tile_box(1, true, arows, 3, box);
    CHECK(box[0] == 2.0f && box[4] == 4.0f && box[8] == 0.25f);
    // an empty tile: never visited, at any qcut
    const float dead[] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float empty[kCutBox];
    cutoff_tile_box(2, false, dead, 2, empty);
    CHECK(empty[0] == finf && empty[4] == -finf && empty[8] == 1.0f);
    const float wave[kCutWaveBox] = {0.0f, 0.0f, 0.0f, 0.0f, 10.0f, 10.0f, 10.0f, 10.0f};
    for (int D = 1; D <= 4; D++) CHECK(!cutoff_visit_d(D, empty, wave, finf) && !cutoff_visit_d(D, empty, wave, 1e30f));
    // a wave without live points visits nothing, not even at R = +infinity -- and neither against an empty tile
    const unsigned char live0[64] = {0};
    const float pts[128] = {0};
    float wbox[kCutWaveBox];
    cutoff_wave_box(2, pts, 64, 0, 64, live0, wbox);
    cutoff_tile_box(2, false, rows, 4, box);
    CHECK(!cutoff_visit_d(2, box, wbox, finf) && !cutoff_visit_d(2, empty, wbox, finf));
    // a wave box over live points only
    unsigned char live[64] = {0};
    float p2[128];
    for (int j = 0; j < 64; j++) {
      p2[j] = (float)j;
      p2[64 + j] = (float)(100 - j);
    }
    live[3] = live[10] = 1;
    cutoff_wave_box(2, p2, 64, 0, 64, live, wbox);
    CHECK(wbox[0] == 3.0f && wbox[4] == 10.0f && wbox[1] == 90.0f && wbox[5] == 97.0f);
    // R = +infinity: every non-empty tile against every live wave, however far
    const float far_[kCutBox] = {1e18f, 1e18f, 0, 0, 2e18f, 2e18f, 0, 0, 1.0f};
    CHECK(cutoff_visit_d(2, far_, wbox, finf) && !cutoff_visit_d(2, far_, wbox, cutoff_qcut(1e6)));
    // qcut exactly on a gap: gap 3 in one observable, q_lb = 9; visited iff q_lb < qcut
    const float t1[kCutBox] = {13.0f, 0, 0, 0, 20.0f, 0, 0, 0, 1.0f};
    const float w1[kCutWaveBox] = {0.0f, 0, 0, 0, 10.0f, 0, 0, 0};
    CHECK(!cutoff_visit_d(1, t1, w1, 9.0f));
    CHECK(cutoff_visit_d(1, t1, w1, std::nextafter(9.0f, finf)));
    CHECK(!cutoff_visit_d(1, t1, w1, std::nextafter(9.0f, 0.0f)));
    // ... and the same gap on the other side, and overlapping boxes (gap 0: always visited)
    const float t2[kCutBox] = {-20.0f, 0, 0, 0, -3.0f, 0, 0, 0, 1.0f};
    CHECK(!cutoff_visit_d(1, t2, w1, 9.0f) && cutoff_visit_d(1, t2, w1, std::nextafter(9.0f, finf)));
    const float t3[kCutBox] = {5.0f, 0, 0, 0, 6.0f, 0, 0, 0, 1.0f};
    CHECK(cutoff_visit_d(1, t3, w1, cutoff_qcut(1.0)));
    // the smallest g scales the bound: g = 0.25 makes the gap count a quarter
    const float t4[kCutBox] = {13.0f, 0, 0, 0, 20.0f, 0, 0, 0, 0.25f};
    CHECK(cutoff_visit_d(1, t4, w1, 9.0f) && !cutoff_visit_d(1, t4, w1, 2.25f));
  }

  // ---- the visit test against the scalar pair arithmetic, randomised: monotone in R, and never rejects a tile that
  // holds a pair below qcut
  {
    std::uniform_real_distribution<float> pos(0.0f, 40.0f), ext(0.0f, 3.0f), gs(0.01f, 100.0f);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f);
    const double Rs[] = {1.0, 1.5, 3.0, 4.0, 6.0, 15.0, inf};
    size_t rejected = 0, visited = 0;
    for (int D = 1; D <= 4; D++) {
      for (int trial = 0; trial < 4000; trial++) {
        const bool adaptive = trial % 2 == 1;
        // a tile of 8 live rows and a wave of 8 live points, compact, at random places (often within a few units)
        const size_t rowlen = (size_t)D + (adaptive ? 2 : 1);
        std::vector<float> rows(8 * rowlen), pts((size_t)D * 8);
        float centre_t[4], centre_w[4];
        for (int d = 0; d < D; d++) {
          centre_t[d] = pos(rng);
          centre_w[d] = trial % 3 == 0 ? centre_t[d] + 4.0f * (unit(rng) - 0.5f) : pos(rng);
        }
        for (size_t j = 0; j < 8; j++) {
          for (int d = 0; d < D; d++) {
            rows[j * rowlen + d] = centre_t[d] + ext(rng);
            pts[(size_t)d * 8 + j] = centre_w[d] + ext(rng);
          }
          if (adaptive) rows[j * rowlen + D] = gs(rng);
          rows[j * rowlen + rowlen - 1] = 1.0f;
        }
        float tbox[kCutBox], wbox[kCutWaveBox];
        const unsigned char live[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        cutoff_tile_box(D, adaptive, rows.data(), 8, tbox);
        cutoff_wave_box(D, pts.data(), 8, 0, 8, live, wbox);
        float qmin = finf;   // the smallest q' the kernel would compute for a pair of this wave and tile
        for (size_t j = 0; j < 8; j++) {
          for (size_t i = 0; i < 8; i++) {
            float p[4];
            for (int d = 0; d < D; d++) p[d] = pts[(size_t)d * 8 + i];
            qmin = std::fmin(qmin, pair_q(D, p, &rows[j * rowlen], adaptive ? rows[j * rowlen + D] : 1.0f));
          }
        }
        bool before = false;
        for (double R : Rs) {
          const float qcut = cutoff_qcut(R);
          const bool v = cutoff_visit_d(D, tbox, wbox, qcut);
          CHECK(v || !before);                 // monotone in R: once visited, visited at every larger R
          before = v;
          if (qmin < qcut) CHECK(v);           // a pair below the cutoff: the tile must be visited
          (v ? visited : rejected)++;
        }
        CHECK(before);                          // R = +infinity visits every non-empty pair of boxes
      }
    }
    CHECK(rejected > 10000 && visited > 10000);   // (both outcomes are exercised)
    std::printf("test_kde_cutoff_plan: %zu visits, %zu rejections\n", visited, rejected);
  }

  // ---- the culled pair sum's split: at least 16 tiles to a workgroup while four workgroups remain to a resident one
  {
    unsigned tps = 2;
    int nsplit = 256;
    cutoff_split(391, 512, 2048, tps, nsplit);      // 1e5 points against 2^17 samples on 256 CUs
    CHECK(tps == 16 && nsplit == 32);
    tps = 2, nsplit = 256;
    cutoff_split(1, 512, 2048, tps, nsplit);        // a few points: the samples' split is what fills the device
    CHECK(tps == 2 && nsplit == 256);
    tps = 103, nsplit = 5;
    cutoff_split(391, 512, 2048, tps, nsplit);      // already coarse: left alone
    CHECK(tps == 103 && nsplit == 5);
    tps = 1, nsplit = 4;
    cutoff_split(100000, 4, 2048, tps, nsplit);     // never more tiles than there are
    CHECK(tps == 4 && nsplit == 1);
    for (unsigned long long pb : {1ull, 7ull, 391ull, 4096ull}) {
      for (unsigned long long nt : {1ull, 3ull, 16ull, 512ull, 1000ull}) {
        tps = 1, nsplit = (int)nt;
        cutoff_split(pb, nt, 2048, tps, nsplit);
        CHECK(tps >= 1 && (unsigned long long)nsplit * tps >= nt && (unsigned long long)(nsplit - 1) * tps < nt);
      }
    }
  }

  // ---- the replay counts what the visit test says
  {
    const float tiles[2 * kCutBox] = {0, 0, 0, 0, 1, 0, 0, 0, 1.0f, 50, 0, 0, 0, 51, 0, 0, 0, 1.0f};
    const float waves[2 * kCutWaveBox] = {0, 0, 0, 0, 1, 0, 0, 0, finf, finf, finf, finf, -finf, -finf, -finf, -finf};
    CHECK(cutoff_replay(1, tiles, 2, waves, 2, cutoff_qcut(3.0)) == 1);
    CHECK(cutoff_replay(1, tiles, 2, waves, 2, finf) == 2);
  }

  if (failures) return 1;
  std::printf("test_kde_cutoff_plan: ok\n");
  return 0;
}
