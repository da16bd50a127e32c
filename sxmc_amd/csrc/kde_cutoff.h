// kde_cutoff.h -- the pure parts of pdfz::EvalKernel's cutoff radius (sxmc_kde_set_cutoff): which R are accepted and
// the f32 cutoff value they give, the spatial sort key and order of table rows and points, the box of a tile of sample
// rows or of a wave of points, and the visit test.  Plain C++ with no device call, so that a stand-alone program can
// include it (tests/cpp/test_kde_cutoff_plan.cpp); the visit test is one inline host/device function, which the culled
// pair kernels (kde_kernels.hip) and a host replay both run: the same operations in the same order, so the same bits.
// The contract is written out in include/sxmc_hip.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SXKDE_HD __host__ __device__
#else
#define SXKDE_HD
#endif

namespace sxkde {

constexpr int kCutMaxDim = 4;                  // SXMC_KDE_MAX_DIM
constexpr int kCutTile = 256;                  // SXMC_KDE_TILE: the culling granule on the sample side
constexpr int kCutWave = 64;                   // ... and on the point side
constexpr int kCutBox = 2 * kCutMaxDim + 1;    // floats to a tile's box: lo[4], hi[4], the smallest g
constexpr int kCutWaveBox = 2 * kCutMaxDim;    // floats to a wave's box: lo[4], hi[4]
constexpr int kCutCounters = 64;               // the visited tiles are counted in this many counters, added on the host
constexpr int kCutCounterStride = 16;          // ... one to a 128-byte line (in 64-bit words)
constexpr unsigned kCutMinTiles = 16;          // tiles to a workgroup of the culled pair sum, where the points allow

// The culled pair sum's split over workgroups, from the plain one's (tiles_per_split, nsplit): every wave pays for its
// tile tests and its count once, so a workgroup takes at least kCutMinTiles tiles while that still leaves four
// workgroups to each of the device's `slots` resident ones (the waves finish at different times: the surplus is what
// balances them).
inline void cutoff_split(unsigned long long pblocks, unsigned long long ntiles, unsigned long long slots,
                         unsigned& tiles_per_split, int& nsplit) {
  unsigned long long tps = tiles_per_split;
  while (tps < kCutMinTiles && tps < ntiles && pblocks * ((ntiles + 2 * tps - 1) / (2 * tps)) >= 4 * slots) tps *= 2;
  tiles_per_split = (unsigned)tps;
  nsplit = (int)((ntiles + tps - 1) / tps);
}

// 0 (off), or 1 <= R <= +infinity; NaN fails every comparison.
inline bool valid_cutoff(double R) { return R == 0.0 || R >= 1.0; }

// qcut = R^2 log2(e) / 2 as the f32 the kernels compare with, rounded UP: a pair whose f32 q' reaches it has
// q' >= R^2 log2(e) / 2 in exact arithmetic as well.  +infinity for R = +infinity (and for an R whose square overflows).
inline float cutoff_qcut(double R) {
  const double q = R * R * 0.72134752044448170;   // log2(e) / 2
  if (!(q < (double)std::numeric_limits<float>::max())) return std::numeric_limits<float>::infinity();
  float f = (float)q;
  if ((double)f < q) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  return f;
}

// ------------------------------------------------------------------------------------ the order
// The key of a row or point with untransformed coordinates x[0 .. D), clamped to [lower, upper] (NaN counts as lower).
// D == 1: the clamped coordinate as a float, mapped to an unsigned that orders as the float does -- a plain sort.
// D > 1: the Morton code of the cell of a fixed grid over the domain, 32 / D bits (16, 10, 8) to an observable.
inline int cutoff_cell_bits(int D) { return D <= 1 ? 32 : 32 / D; }

inline uint32_t cutoff_float_bits(float f) {
  uint32_t u;
  static_assert(sizeof u == sizeof f, "float is 32 bits");
  std::memcpy(&u, &f, sizeof u);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

inline uint32_t cutoff_key(int D, const double* x, const double* lower, const double* upper) {
  if (D == 1) {
    double v = x[0];
    if (!(v >= lower[0])) v = lower[0];
    if (v > upper[0]) v = upper[0];
    return cutoff_float_bits((float)v);
  }
  const int bits = cutoff_cell_bits(D);
  const uint32_t ncell = 1u << bits;
  uint32_t cell[kCutMaxDim] = {0, 0, 0, 0};
  for (int d = 0; d < D; d++) {
    double t = (x[d] - lower[d]) / (upper[d] - lower[d]);
    if (!(t >= 0.0)) t = 0.0;
    if (t > 1.0) t = 1.0;
    const double c = std::floor(t * (double)ncell);
    cell[d] = c >= (double)ncell ? ncell - 1u : (uint32_t)c;
  }
  uint32_t key = 0;
  for (int b = bits - 1; b >= 0; b--) {
    for (int d = 0; d < D; d++) key = (key << 1) | ((cell[d] >> b) & 1u);
  }
  return key;
}

// The order of n keys: stable, ties by index.  order[k] = the index that comes k-th.
inline std::vector<uint32_t> cutoff_order(const std::vector<uint32_t>& keys) {
  std::vector<uint32_t> order(keys.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  return order;
}

// The permutation of the npad (a multiple of kCutTile) sample rows of a table: its nsamples rows by key, the padding
// after them.  x: the untransformed observables, row i at x[i * stride .. + D).
inline std::vector<uint32_t> cutoff_sample_order(int D, const float* x, size_t stride, size_t nsamples, size_t npad,
                                                 const double* lower, const double* upper) {
  std::vector<uint32_t> keys(nsamples);
  for (size_t i = 0; i < nsamples; i++) {
    double v[kCutMaxDim];
    for (int d = 0; d < D; d++) v[d] = (double)x[i * stride + (size_t)d];
    keys[i] = cutoff_key(D, v, lower, upper);
  }
  std::vector<uint32_t> order = cutoff_order(keys);
  for (size_t i = nsamples; i < npad; i++) order.push_back((uint32_t)i);
  return order;
}

// The order of n evaluation points: the live ones (code 0) by key, the others after them in their own order.
inline std::vector<uint32_t> cutoff_point_order(int D, const float* points, size_t n, const int* codes,
                                                const double* lower, const double* upper, size_t* nlive) {
  const size_t row = (size_t)D + 1;
  std::vector<uint32_t> live, dead, keys;
  for (size_t i = 0; i < n; i++) {
    if (codes[i] != 0) {
      dead.push_back((uint32_t)i);
      continue;
    }
    double v[kCutMaxDim];
    for (int d = 0; d < D; d++) v[d] = (double)points[i * row + (size_t)d];
    live.push_back((uint32_t)i);
    keys.push_back(cutoff_key(D, v, lower, upper));
  }
  const std::vector<uint32_t> o = cutoff_order(keys);
  std::vector<uint32_t> order;
  order.reserve(n);
  for (uint32_t k : o) order.push_back(live[k]);
  order.insert(order.end(), dead.begin(), dead.end());
  if (nlive) *nlive = live.size();
  return order;
}

// ------------------------------------------------------------------------------------ the boxes
// An empty box: no pair, so no gap is finite and the visit test fails at every qcut, +infinity included.
inline void cutoff_empty_box(float* lo, float* hi) {
  for (int d = 0; d < kCutMaxDim; d++) {
    lo[d] = std::numeric_limits<float>::infinity();
    hi[d] = -std::numeric_limits<float>::infinity();
  }
}

// The box of one tile of sample rows (rowlen = D + 1 floats, or D + 2 for an adaptive evaluator: c_d, [g,] weight): min
// and max of c_d over the rows with weight > 0 and the smallest g among them (1 when fixed or empty).
inline void cutoff_tile_box(int D, bool adaptive, const float* rows, size_t nrows, float* box) {
  const size_t rowlen = (size_t)D + (adaptive ? 2 : 1);
  cutoff_empty_box(box, box + kCutMaxDim);
  float g = std::numeric_limits<float>::infinity();
  for (size_t j = 0; j < nrows; j++) {
    const float* r = rows + j * rowlen;
    if (!(r[rowlen - 1] > 0.0f)) continue;
    for (int d = 0; d < D; d++) {
      box[d] = std::fmin(box[d], r[d]);
      box[kCutMaxDim + d] = std::fmax(box[kCutMaxDim + d], r[d]);
    }
    if (adaptive) g = std::fmin(g, r[D]);
  }
  box[2 * kCutMaxDim] = (adaptive && g < std::numeric_limits<float>::infinity()) ? g : 1.0f;
}

// The box of one wave of sorted points: pts [D][pitch] scaled coordinates, live[j] whether sorted point j counts.
inline void cutoff_wave_box(int D, const float* pts, size_t pitch, size_t first, size_t count, const unsigned char* live,
                            float* box) {
  cutoff_empty_box(box, box + kCutMaxDim);
  for (size_t j = first; j < first + count; j++) {
    if (!live[j]) continue;
    for (int d = 0; d < D; d++) {
      const float c = pts[(size_t)d * pitch + j];
      box[d] = std::fmin(box[d], c);
      box[kCutMaxDim + d] = std::fmax(box[kCutMaxDim + d], c);
    }
  }
}

// ------------------------------------------------------------------------------------ the visit test
// q_lb of a wave of points against a tile of samples: per observable the gap between the two boxes,
//   gap_d = max(0, tile_lo_d - wave_hi_d, wave_lo_d - tile_hi_d),
// then the pair kernels' own sequence on it -- the square of the first, a fused multiply-add per further observable,
// times the tile's smallest g.  Every pair of the wave and the tile has |c_pd - c_id| >= gap_d before rounding, each
// operation rounds monotonically, and g_i >= g_min > 0: so the kernel's f32 q' of every such pair is >= q_lb, with no
// margin.  A tile is visited iff q_lb < qcut; with an empty box on either side a gap is +infinity and so is q_lb.
template <int D>
SXKDE_HD inline float cutoff_q_lb(const float* tile_lo, const float* tile_hi, float g_min, const float* wave_lo,
                                  const float* wave_hi) {
  float q = 0.0f;
  for (int d = 0; d < D; d++) {
    const float a = tile_lo[d] - wave_hi[d];
    const float b = wave_lo[d] - tile_hi[d];
    float gap = a > b ? a : b;
    gap = gap > 0.0f ? gap : 0.0f;
    q = d == 0 ? gap * gap : __builtin_fmaf(gap, gap, q);
  }
  return g_min * q;
}

template <int D>
SXKDE_HD inline bool cutoff_visit(const float* tile_lo, const float* tile_hi, float g_min, const float* wave_lo,
                                  const float* wave_hi, float qcut) {
  return cutoff_q_lb<D>(tile_lo, tile_hi, g_min, wave_lo, wave_hi) < qcut;
}

// the same by a run-time D (the host replay)
inline bool cutoff_visit_d(int D, const float* tile_box, const float* wave_box, float qcut) {
  const float *tl = tile_box, *th = tile_box + kCutMaxDim, *wl = wave_box, *wh = wave_box + kCutMaxDim;
  const float g = tile_box[2 * kCutMaxDim];
  switch (D) {
    case 1: return cutoff_visit<1>(tl, th, g, wl, wh, qcut);
    case 2: return cutoff_visit<2>(tl, th, g, wl, wh, qcut);
    case 3: return cutoff_visit<3>(tl, th, g, wl, wh, qcut);
    case 4: return cutoff_visit<4>(tl, th, g, wl, wh, qcut);
    default: return false;
  }
}

// The tiles the waves of a point plan visit in all: what the device counts (sxmc_kde_cutoff_stats).
inline unsigned long long cutoff_replay(int D, const float* tile_boxes, size_t ntiles, const float* wave_boxes,
                                        size_t nwaves, float qcut) {
  unsigned long long n = 0;
  for (size_t w = 0; w < nwaves; w++) {
    for (size_t t = 0; t < ntiles; t++) {
      n += cutoff_visit_d(D, tile_boxes + t * kCutBox, wave_boxes + w * kCutWaveBox, qcut) ? 1u : 0u;
    }
  }
  return n;
}

}  // namespace sxkde
