// kde_kernels.hip -- gfx950 kernels of pdfz::EvalKernel, the kernel-density PDF (sxmc_kde_*, sxmc_kde.cpp).
//
// One evaluation is three launches on the evaluator's stream:
//   kde_prepass   one lane per SXMC_VEC samples: the systematics in f64 (apply_op of fill_kernels.inc.h, the fill's own
//                 arithmetic), the domain test, the in-domain count (integer atomics: the norm), and per sample the
//                 scaled coordinates c_d = (x_d - lower_d) * sqrt(log2(e) / 2) / h_d in f32 and the weight
//                 w = 1 / prod_d [Phi((upper_d - x_d) / h_d) - Phi((lower_d - x_d) / h_d)] (f64 with erfc), or 0 and
//                 c = 0 outside the domain.  Rows of D + 1 floats, in table order.
//   kde_pairs     one lane per evaluation point, the samples wave-uniform (scalar loads into SGPR operands):
//                 sum_i w_i * exp2(-sum_d (c_pd - c_id)^2), in f32 within a tile of kKdeTile samples and in f64 across
//                 tiles.  When the points alone do not fill the GPU the samples are split across workgroups
//                 (blockIdx.y), each writing its own partial sum.
//   kde_combine   per point the partials added in split order, times 1 / (norm (2 pi)^(D/2) prod h) in f64; the point
//                 codes of EvalHist::SetEvalPoints (-1 NaN, -2 zero); norm == 0 gives NaN.
// No floating-point atomics and no order that depends on timing: two evaluations give the same bits.
// Sampling (sxmc_kde_random_sample) and the projection onto one observable (sxmc_kde_project) follow the evaluation.
// A kernel templated on the observables D (and on ADAPT) is picked from the run-time values by kde_for_dim /
// kde_for_dim_adapt below, the one place that does so.
//
// Adaptive evaluators (bandwidth sensitivity > 0, sxmc_kde_create_adaptive) give every table row i a factor lambda_i on
// the bandwidths, fixed at construction by kde_pilot (at the end of this file) and kept in d_lambda.  Their prepass
// (ADAPT = true) writes rows of D + 2 floats -- the same c_d in units of the global h_d, g_i = 1 / lambda_i^2 and
// W_i = w_i / lambda_i^D with the mass taken at h_d lambda_i -- and kde_pairs<D, true> sums W_i exp2(-g_i q); the
// sampler and the projection read lambda in f64.  A fixed-bandwidth evaluator never runs an ADAPT instantiation.
//
// Bandwidth cross-validation (sxmc_kde_cv_scores / sxmc_kde_cv_select) scores K candidate bandwidth vectors in one f64
// pass over the pairs of the untransformed in-domain rows: kde_cv_weights, kde_cv_pairs and kde_cv_combine, last in
// this file.  It reads the table only and leaves the rows of the last evaluation alone.
//
// A cutoff radius (sxmc_kde_set_cutoff, R > 0) puts kde_cutoff_gather between the prepass and the pair sum, replaces
// the latter by kde_pairs_cutoff (both after kde_combine below; the pure parts in kde_cutoff.h) and gives kde_combine
// the order of the sorted points.  At R = 0 neither runs and kde_combine takes no order.
//
// Weighted Monte Carlo samples (sxmc_kde_create_weighted: one integer multiplicity m_i per table row) fold m_i into the
// row's weight in the prepass, so kde_pairs, kde_pairs_cutoff, kde_cutoff_gather and kde_combine are the same code for
// them.  What reads multiplicities is an instantiation or a sibling of its own, made from the one source by a
// compile-time WEIGHTED -- kde_prepass, kde_project_prep and kde_sample (with kde_mflag) over a KdeMult / KdePick,
// kde_pilot_combine_weighted: an evaluator without multiplicities launches the kernels it launched before them,
// instruction for instruction.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "nll_device.h"

#include "fill_kernels.inc.h"
#include "kde_cutoff.h"
#include "kde_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace sxfill;

constexpr int kKdeTile = SXMC_KDE_TILE;   // samples per f32 partial sum (the sample rows are padded to a multiple)
constexpr int kKdeBlock = 256;

// The one run-time to compile-time dispatch of this file: f(std::integral_constant<int, N>{}) for N = D in
// [1, SXMC_KDE_MAX_DIM] (kde_for_dim), or in [1, MAX] (kde_for_range: the prepass's slots), else hipErrorInvalidValue.
template <int MAX, class F>
hipError_t kde_for_range(int n, F&& f) {
  if constexpr (MAX >= 1) {
    if (n == MAX) return f(std::integral_constant<int, MAX>{});
    return kde_for_range<MAX - 1>(n, std::forward<F>(f));
  }
  return hipErrorInvalidValue;
}
template <class F>
hipError_t kde_for_dim(int D, F&& f) {
  return kde_for_range<SXMC_KDE_MAX_DIM>(D, std::forward<F>(f));
}
// ... and f(dim, std::bool_constant<adaptive>{})
template <class F>
hipError_t kde_for_dim_adapt(int D, bool adaptive, F&& f) {
  return kde_for_dim(D, [&](auto dim) { return adaptive ? f(dim, std::true_type{}) : f(dim, std::false_type{}); });
}

// Weightedness is a compile-time fact of a kernel below, carried by a trailing argument pack: empty for an evaluator
// without multiplicities -- whose instantiation then has the arguments, the kernel-argument layout and the instructions
// it had before weights existed -- or one KdeMult (the sampler: one KdePick).  WEIGHTED = the pack is not empty.
struct KdeMult {
  const unsigned* __restrict__ p;   // [npad] the rows' multiplicities, 0 in the padding
};
template <class T>
__device__ __forceinline__ const T& kde_only(const T& t) {
  return t;
}
// ... and nothing else: no element, or exactly one of type T
template <class T, class... PACK>
constexpr bool kde_pack_is() {
  return sizeof...(PACK) == 0 || (sizeof...(PACK) == 1 && (std::is_same<T, PACK>::value && ...));
}

// The prepass, written once.  WEIGHTED (sxmc_kde_create_weighted; `mult`: [npad] the rows' multiplicities, 0 in the
// padding, else unused): a row counts m_i in the norm and its weight is (float)((double)m_i / mass) -- the multiplicity
// folded into the number the pair sum multiplies by, so that nothing after the prepass knows of it.  The four
// multiplicities of a lane's SXMC_VEC rows come in one 16-byte load.
template <int NSLOT, bool ADAPT, class... MULT>
__global__ __launch_bounds__(kKdeBlock) void kde_prepass_kernel(const SxSignalDesc d, const SxKdeArgs a,
                                                                const MULT... mult) {
  static_assert(kde_pack_is<KdeMult, MULT...>(), "the pack is empty or one KdeMult");
  constexpr bool WEIGHTED = sizeof...(MULT) == 1;
  const unsigned tid = threadIdx.x;
  const unsigned lane = tid & (kWave - 1);
  const unsigned long long v = (unsigned long long)blockIdx.x * kKdeBlock + tid;
  // the coefficients, one per lane, read back with v_readlane by apply_op (every lane of the wave stays to the end)
  double coef = 0.0;
  if ((int)lane < d.ncoef) coef = d.params[(long)d.coef_par[lane] * d.param_stride];
  const unsigned long long vc = v < d.nvec ? v : d.nvec - 1;
  double f[NSLOT][SXMC_VEC];
#pragma unroll
  for (int k = 0; k < NSLOT; k++) {
    const float* col = d.cols + (unsigned long long)d.slot_col[k] * d.col_pitch + vc * SXMC_VEC;
#pragma unroll
    for (int q = 0; q < SXMC_VEC; q++) f[k][q] = (double)col[q];
  }
  for (int s = 0; s < d.nsyst; s++) apply_op<NSLOT>(f, pack_opword(d.syst[s]), coef);

  constexpr int D = NSLOT < SXMC_KDE_MAX_DIM ? NSLOT : SXMC_KDE_MAX_DIM;
  unsigned mq[SXMC_VEC] = {0u, 0u, 0u, 0u};   // (WEIGHTED) what each of the lane's rows counts for
  if constexpr (WEIGHTED) {
    static_assert(SXMC_VEC == 4, "one 16-byte load of multiplicities per lane");
    // (lanes past the padded rows read unit 0: their rows fail the domain test)
    const unsigned long long vm = v < a.npad / SXMC_VEC ? v : 0ull;
    const uint4 m4 = *reinterpret_cast<const uint4*>(kde_only(mult...).p + vm * SXMC_VEC);
    mq[0] = m4.x;
    mq[1] = m4.y;
    mq[2] = m4.z;
    mq[3] = m4.w;
  }
  unsigned cnt = 0;
#pragma unroll
  for (int q = 0; q < SXMC_VEC; q++) {
    const unsigned long long i = v * SXMC_VEC + q;
    // pdfz.cpp:388-398: lower <= x < upper, written so that NaN fails
    bool in = v < d.nvec && i < d.nsamples;
#pragma unroll
    for (int k = 0; k < D; k++) {
      if (k < d.nobs) in = in && (f[k][q] >= a.lower[k]) && (f[k][q] < a.upper[k]);
    }
    if constexpr (WEIGHTED) cnt += in ? mq[q] : 0u;
    else cnt += in ? 1u : 0u;
    if (i < a.npad) {
      double mass = 1.0;
      float* row = a.rows + i * (unsigned long long)(d.nobs + (ADAPT ? 2 : 1));
      double lam = 1.0, lam_pow = 1.0;   // (ADAPT) the row's factor and lambda^D
      if constexpr (ADAPT) lam = a.lambda[i];
#pragma unroll
      for (int k = 0; k < D; k++) {
        if (k >= d.nobs) continue;
        const double x = in ? f[k][q] : a.lower[k];
        double r = a.inv_h_sqrt2[k];
        if constexpr (ADAPT) {
          r = r / lam;   // 1 / (h lambda sqrt 2)
          lam_pow = lam_pow * lam;
        }
        mass = mass * sxkde::truncation_mass(x, a.lower[k], a.upper[k], r);
        row[k] = in ? (float)((x - a.lower[k]) * a.cscale[k]) : 0.0f;
      }
      double one = 1.0;   // the numerator of the row's weight: (WEIGHTED) its multiplicity, 0 leaving the weight 0
      if constexpr (WEIGHTED) one = (double)mq[q];
      if constexpr (ADAPT) {
        row[d.nobs] = (float)(1.0 / (lam * lam));
        row[d.nobs + 1] = in ? (float)(one / (mass * lam_pow)) : 0.0f;
      } else {
        row[d.nobs] = in ? (float)(one / mass) : 0.0f;
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
  if (lane == 0 && cnt != 0u) __hip_atomic_fetch_add(a.norm, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The pair sum's inner loop, written once: the f32 sum of one tile's terms at one point.  Rows of D + 1 floats (c_d, w)
// and the term w exp2(-q), or (ADAPT) of D + 2 floats (c_d, g = 1 / lambda^2, W = w / lambda^D) and the term
// W exp2(-g q): one multiply more per pair.
template <int D, bool ADAPT>
__device__ __forceinline__ float kde_tile_sum(const float (&p)[D], const float* __restrict__ s) {
  constexpr int kRow = D + (ADAPT ? 2 : 1);
  float acc = 0.0f;
#pragma unroll 16
  for (int j = 0; j < kKdeTile; j++) {
    const float* r = s + j * kRow;
    const float a0 = p[0] - r[0];
    float q = a0 * a0;
#pragma unroll
    for (int k = 1; k < D; k++) {
      const float ak = p[k] - r[k];
      q = __builtin_fmaf(ak, ak, q);
    }
    if constexpr (ADAPT) acc = __builtin_fmaf(r[D + 1], __builtin_amdgcn_exp2f(-(r[D] * q)), acc);
    else acc = __builtin_fmaf(r[D], __builtin_amdgcn_exp2f(-q), acc);
  }
  return acc;
}

// One lane per point; every lane of the grid runs the full trip count (points are padded with zeros), so the sample
// rows are read at wave-uniform addresses: scalar loads, SGPR operands of the vector instructions.
template <int D, bool ADAPT>
__global__ __launch_bounds__(kKdeBlock) void kde_pairs_kernel(const float* __restrict__ pts, unsigned long long pitch,
                                                              const float* __restrict__ rows, unsigned tiles_per_split,
                                                              unsigned ntiles, double* __restrict__ part) {
  constexpr int kRow = D + (ADAPT ? 2 : 1);
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  float p[D];
#pragma unroll
  for (int k = 0; k < D; k++) p[k] = pts[(unsigned long long)k * pitch + i];
  const unsigned t0 = blockIdx.y * tiles_per_split;
  const unsigned t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  double sum = 0.0;
  for (unsigned t = t0; t < t1; t++) {
    sum += (double)kde_tile_sum<D, ADAPT>(p, rows + (unsigned long long)t * kKdeTile * kRow);
  }
  part[(unsigned long long)blockIdx.y * pitch + i] = sum;
}

// One lane per place j of the partial sums, which are added in split order; the value goes to point order[j] -- the
// caller's point that stands at sorted place j (a cutoff) -- or to point j when order is null.  codes: in the caller's
// order.
__global__ __launch_bounds__(kKdeBlock) void kde_combine_kernel(const double* __restrict__ part, unsigned long long pitch,
                                                                int nsplit, unsigned long long npoints,
                                                                const int* __restrict__ codes,
                                                                const unsigned* __restrict__ order,
                                                                const unsigned* __restrict__ norm, double prefactor,
                                                                float* __restrict__ out, long stride) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (j >= npoints) return;
  const unsigned long long i = order ? order[j] : j;
  const int code = codes[i];
  float v;
  if (code == -2) {
    v = 0.0f;                              // in the domain, another data set (pdfz.cpp:423-434)
  } else if (code < 0) {
    v = __int_as_float(0x7fc00000);        // outside the domain
  } else {
    double s = 0.0;
    for (int k = 0; k < nsplit; k++) s += part[(unsigned long long)k * pitch + j];
    const unsigned n = *norm;
    v = n == 0u ? __int_as_float(0x7fc00000) : (float)(s * prefactor / (double)n);
  }
  out[stride * (long)i] = v;
}

// ------------------------------------------------------------------------------------ cutoff radius (sxmc_kde_set_cutoff)
// With a cutoff the pair sum runs on a second copy of the prepass's rows in the spatial order of kde_cutoff.h, and on
// points sorted by the same key: kde_cutoff_gather and kde_pairs_cutoff below, and kde_combine with the points' order.
// The prepass, the sampler and the projection are untouched and keep the rows in table order.

// One workgroup per tile: row perm[k] of the prepass's rows goes to place k of the sorted rows, and the tile's box --
// min and max of c_d over its rows with weight > 0, and the smallest g when adaptive -- to box[tile] (kCutBox floats;
// empty: lo = +inf, hi = -inf, g = 1).  perm is a permutation of [0, npad), the grid npad / 256 workgroups.
template <int D, bool ADAPT>
__global__ __launch_bounds__(kKdeBlock) void kde_cutoff_gather_kernel(const float* __restrict__ rows,
                                                                      const unsigned* __restrict__ perm,
                                                                      float* __restrict__ sorted,
                                                                      float* __restrict__ box) {
  constexpr int kRow = D + (ADAPT ? 2 : 1);
  constexpr float kInf = __builtin_huge_valf();
  __shared__ float red[kKdeBlock / kWave][2 * D + 1];
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const unsigned long long k = (unsigned long long)blockIdx.x * kKdeBlock + tid;
  const float* src = rows + (unsigned long long)perm[k] * kRow;
  float* dst = sorted + k * kRow;
  float r[kRow];
#pragma unroll
  for (int j = 0; j < kRow; j++) {
    r[j] = src[j];
    dst[j] = r[j];
  }
  const bool live = r[kRow - 1] > 0.0f;
  float lo[D], hi[D], g = kInf;
#pragma unroll
  for (int d = 0; d < D; d++) {
    lo[d] = live ? r[d] : kInf;
    hi[d] = live ? r[d] : -kInf;
  }
  if constexpr (ADAPT) g = live ? r[D] : kInf;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      lo[d] = fminf(lo[d], __shfl_down(lo[d], off, kWave));
      hi[d] = fmaxf(hi[d], __shfl_down(hi[d], off, kWave));
    }
    if constexpr (ADAPT) g = fminf(g, __shfl_down(g, off, kWave));
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      red[wv][d] = lo[d];
      red[wv][D + d] = hi[d];
    }
    red[wv][2 * D] = g;
  }
  __syncthreads();
  if (tid == 0) {
    float* b = box + (unsigned long long)blockIdx.x * sxkde::kCutBox;
#pragma unroll
    for (int d = 0; d < sxkde::kCutMaxDim; d++) {
      float l = kInf, h = -kInf;   // (the observables the evaluator does not have keep an empty range)
      for (int w = 0; w < kKdeBlock / kWave && d < D; w++) {
        l = fminf(l, red[w][d % D]);
        h = fmaxf(h, red[w][D + d % D]);
      }
      b[d] = l;
      b[sxkde::kCutMaxDim + d] = h;
    }
    float gm = kInf;
    for (int w = 0; w < kKdeBlock / kWave; w++) gm = fminf(gm, red[w][2 * D]);
    b[2 * sxkde::kCutMaxDim] = (ADAPT && gm < kInf) ? gm : 1.0f;
  }
}

// The culled pair sum: kde_pairs_kernel's shape on the sorted points and rows, but each wave visits, of its split's
// tiles, only those whose box lies within the cutoff of the wave's own box (sxkde::cutoff_visit, one lane per tile, 64
// tiles at a time; the set bits of the ballot walked in tile order with the tile number made provably uniform, so that
// the rows still come through scalar loads).  f32 within a tile, f64 across the visited tiles in tile order.  No
// barrier: the waves of a workgroup take different tile lists.  Each wave adds the tiles it visited to one of
// sxkde::kCutCounters counters (one integer atomic; one address would serialise every wave of the grid).
template <int D, bool ADAPT>
__global__ __launch_bounds__(kKdeBlock) void kde_pairs_cutoff_kernel(const float* __restrict__ pts,
                                                                     unsigned long long pitch,
                                                                     const float* __restrict__ rows,
                                                                     const float* __restrict__ tile_box,
                                                                     const float* __restrict__ wave_box,
                                                                     unsigned tiles_per_split, unsigned ntiles,
                                                                     float qcut, double* __restrict__ part,
                                                                     unsigned long long* __restrict__ visited) {
  constexpr int kRow = D + (ADAPT ? 2 : 1);
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & (kWave - 1);
  float p[D];
#pragma unroll
  for (int k = 0; k < D; k++) p[k] = pts[(unsigned long long)k * pitch + i];
  // the wave's own box (the wave number is the same in every lane: made so for the compiler too)
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kKdeBlock / kWave) + threadIdx.x / kWave);
  const float* wb = wave_box + (unsigned long long)wave * sxkde::kCutWaveBox;
  float wlo[D], whi[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    wlo[k] = wb[k];
    whi[k] = wb[sxkde::kCutMaxDim + k];
  }
  const unsigned t0 = blockIdx.y * tiles_per_split;
  const unsigned t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  double sum = 0.0;
  unsigned nvisited = 0;
  for (unsigned base = t0; base < t1; base += kWave) {
    const unsigned t = base + lane;
    bool visit = false;
    if (t < t1) {
      const float* b = tile_box + (unsigned long long)t * sxkde::kCutBox;
      float tlo[D], thi[D];
#pragma unroll
      for (int k = 0; k < D; k++) {
        tlo[k] = b[k];
        thi[k] = b[sxkde::kCutMaxDim + k];
      }
      visit = sxkde::cutoff_visit<D>(tlo, thi, b[2 * sxkde::kCutMaxDim], wlo, whi, qcut);
    }
    unsigned long long mask = __builtin_amdgcn_ballot_w64(visit);
    nvisited += (unsigned)__builtin_popcountll(mask);
    while (mask != 0ull) {
      const unsigned tt = __builtin_amdgcn_readfirstlane(base + (unsigned)__builtin_ctzll(mask));
      mask &= mask - 1ull;
      sum += (double)kde_tile_sum<D, ADAPT>(p, rows + (unsigned long long)tt * kKdeTile * kRow);
    }
  }
  part[(unsigned long long)blockIdx.y * pitch + i] = sum;
  if (lane == 0 && nvisited != 0u) {
    unsigned long long* counter =
        visited + ((blockIdx.x + blockIdx.y) % sxkde::kCutCounters) * (unsigned)sxkde::kCutCounterStride;
    __hip_atomic_fetch_add(counter, (unsigned long long)nvisited, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

hipError_t sx_kde_prepass(const SxSignalDesc& d, const SxKdeArgs& a, const unsigned* mult, hipStream_t s) {
  const unsigned long long nvec = a.npad / SXMC_VEC;
  const unsigned grid = (unsigned)((nvec + kKdeBlock - 1) / kKdeBlock);
  if (grid == 0) return hipSuccess;
  return kde_for_range<7>(d.nslot, [&](auto nslot) {
    constexpr int N = decltype(nslot)::value;
    const dim3 g(grid), b(kKdeBlock);
    if (mult) {
      const KdeMult m{mult};
      if (a.lambda) hipLaunchKernelGGL((kde_prepass_kernel<N, true, KdeMult>), g, b, 0, s, d, a, m);
      else hipLaunchKernelGGL((kde_prepass_kernel<N, false, KdeMult>), g, b, 0, s, d, a, m);
    } else if (a.lambda) {
      hipLaunchKernelGGL((kde_prepass_kernel<N, true>), g, b, 0, s, d, a);
    } else {
      hipLaunchKernelGGL((kde_prepass_kernel<N, false>), g, b, 0, s, d, a);
    }
    return hipGetLastError();
  });
}

hipError_t sx_kde_pairs(int D, bool adaptive, const float* pts, unsigned long long pitch, const float* rows,
                        unsigned tiles_per_split, unsigned ntiles, int nsplit, double* part, hipStream_t s) {
  const dim3 grid((unsigned)(pitch / kKdeBlock), (unsigned)nsplit);
  return kde_for_dim_adapt(D, adaptive, [&](auto dim, auto adapt) {
    hipLaunchKernelGGL((kde_pairs_kernel<decltype(dim)::value, decltype(adapt)::value>), grid, dim3(kKdeBlock), 0, s,
                       pts, pitch, rows, tiles_per_split, ntiles, part);
    return hipGetLastError();
  });
}

hipError_t sx_kde_combine(const double* part, unsigned long long pitch, int nsplit, unsigned long long npoints,
                          const int* codes, const unsigned* order, const unsigned* norm, double prefactor, float* out,
                          long stride, hipStream_t s) {
  if (npoints == 0) return hipSuccess;
  const unsigned grid = (unsigned)((npoints + kKdeBlock - 1) / kKdeBlock);
  hipLaunchKernelGGL(kde_combine_kernel, dim3(grid), dim3(kKdeBlock), 0, s, part, pitch, nsplit, npoints, codes, order,
                     norm, prefactor, out, stride);
  return hipGetLastError();
}

hipError_t sx_kde_cutoff_gather(int D, bool adaptive, const float* rows, const unsigned* perm, unsigned ntiles,
                                float* sorted, float* box, hipStream_t s) {
  if (ntiles == 0) return hipSuccess;
  return kde_for_dim_adapt(D, adaptive, [&](auto dim, auto adapt) {
    hipLaunchKernelGGL((kde_cutoff_gather_kernel<decltype(dim)::value, decltype(adapt)::value>), dim3(ntiles),
                       dim3(kKdeBlock), 0, s, rows, perm, sorted, box);
    return hipGetLastError();
  });
}

hipError_t sx_kde_pairs_cutoff(int D, bool adaptive, const float* pts, unsigned long long pitch, const float* rows,
                               const float* tile_box, const float* wave_box, unsigned tiles_per_split, unsigned ntiles,
                               int nsplit, float qcut, double* part, unsigned long long* visited, hipStream_t s) {
  const dim3 grid((unsigned)(pitch / kKdeBlock), (unsigned)nsplit);
  return kde_for_dim_adapt(D, adaptive, [&](auto dim, auto adapt) {
    hipLaunchKernelGGL((kde_pairs_cutoff_kernel<decltype(dim)::value, decltype(adapt)::value>), grid, dim3(kKdeBlock),
                       0, s, pts, pitch, rows, tile_box, wave_box, tiles_per_split, ntiles, qcut, part, visited);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------ sampling (sxmc_kde_random_sample)
// Draws from the PDF of the evaluator's last evaluation, which the rows the prepass left describe: an in-domain sample
// has weight > 0, every other row 0.  (1) kde_flag + an inclusive scan (sx_inclusive_sum_u32) + kde_scatter list the in-domain rows in table
// order; (2) kde_sample, one lane per event: a row picked uniformly from that list, then per observable a Gaussian
// around its centre truncated to [lower, upper), drawn by the inverse CDF in f64.
namespace {

// rowlen floats to a row, the weight last (D + 1, or D + 2 for an adaptive evaluator)
__global__ __launch_bounds__(kKdeBlock) void kde_flag_kernel(const float* __restrict__ rows, int rowlen,
                                                             unsigned long long npad, unsigned* __restrict__ flag) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= npad) return;
  flag[i] = rows[i * (unsigned long long)rowlen + (unsigned long long)(rowlen - 1)] > 0.0f ? 1u : 0u;
}

__global__ __launch_bounds__(kKdeBlock) void kde_scatter_kernel(const unsigned* __restrict__ flag,
                                                                const unsigned* __restrict__ pos,
                                                                unsigned long long npad, unsigned* __restrict__ idx) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= npad) return;
  if (flag[i]) idx[pos[i] - 1u] = (unsigned)i;   // pos: inclusive prefix sum of flag, so pos[i] >= 1 here
}

// Phi(z) = erfc(-z / sqrt 2) / 2, accurate in the lower tail; Phi^-1(p) = -sqrt 2 erfcinv(2 p), accurate for small p
__device__ __forceinline__ double kde_phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752); }
__device__ __forceinline__ double kde_phi_inv(double p) { return -1.4142135623730950 * erfcinv(2.0 * p); }

// (WEIGHTED) the multiplicities' scan: one lane per row, m_i where the last evaluation left the row a weight > 0, else 0
__global__ __launch_bounds__(kKdeBlock) void kde_mflag_kernel(const float* __restrict__ rows, int rowlen,
                                                              unsigned long long npad,
                                                              const unsigned* __restrict__ mult,
                                                              unsigned* __restrict__ flag) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= npad) return;
  flag[i] = rows[i * (unsigned long long)rowlen + (unsigned long long)(rowlen - 1)] > 0.0f ? mult[i] : 0u;
}

// What a WEIGHTED sampler picks from (its trailing argument, as KdeMult above): cum = C, the inclusive prefix sum over
// all npad rows of the live rows' multiplicities.
struct KdePick {
  const unsigned* __restrict__ cum;
  unsigned npad;
};

// The sampler, written once.  Unweighted: idx lists the n in-domain rows and the first word picks place (word n) >> 32.
// WEIGHTED: idx is unused and n is T, the last entry of C (the norm, <= 2^32 - 1: the 64-bit product cannot wrap);
// target = (word T) >> 32 < T and the row picked is the first whose C exceeds target -- a live row, since C only grows
// there.
template <int D, bool ADAPT, class... PICK>
__global__ __launch_bounds__(kKdeBlock) void kde_sample_kernel(const float* __restrict__ rows,
                                                               const double* __restrict__ lambda,
                                                               const unsigned* __restrict__ idx, unsigned n,
                                                               const SxKdeSampleArgs g, unsigned long long seed,
                                                               unsigned long long nevents, float* __restrict__ out,
                                                               unsigned* __restrict__ exhausted,
                                                               const PICK... pick) {
  static_assert(kde_pack_is<KdePick, PICK...>(), "the pack is empty or one KdePick");
  constexpr bool WEIGHTED = sizeof...(PICK) == 1;
  const unsigned long long step = (unsigned long long)gridDim.x * kKdeBlock;
  for (unsigned long long e = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x; e < nevents; e += step) {
    float x[D];
    for (unsigned attempt = 0; attempt < 1024; attempt++) {
      // five words per attempt: two Philox blocks, counters (e, 2 attempt) and (e, 2 attempt + 1)
      const sxdev::Philox4 r0 = sxdev::philox4x32_10(e, 2ull * attempt, seed);
      const sxdev::Philox4 r1 = sxdev::philox4x32_10(e, 2ull * attempt + 1ull, seed);
      const unsigned u[4] = {r0.y, r0.z, r0.w, r1.x};
      unsigned i;
      if constexpr (WEIGHTED) {
        const unsigned target = (unsigned)(((unsigned long long)r0.x * n) >> 32);   // < T
        const KdePick& c = kde_only(pick...);
        unsigned lo = 0u, hi = c.npad - 1u;   // (C[npad - 1] = T > target: the search ends inside the table)
        while (lo < hi) {
          const unsigned mid = lo + (hi - lo) / 2u;
          if (c.cum[mid] > target) hi = mid;
          else lo = mid + 1u;
        }
        i = lo;
      } else {
        i = idx[(unsigned)(((unsigned long long)r0.x * n) >> 32)];   // uniform over the n rows
      }
      const float* row = rows + (unsigned long long)i * (D + (ADAPT ? 2 : 1));
      double lam = 1.0;   // (ADAPT) the picked row's factor on every bandwidth
      if constexpr (ADAPT) lam = lambda[i];
      bool ok = true;
#pragma unroll
      for (int k = 0; k < D; k++) {
        const double s = g.lower[k] + (double)row[k] * g.inv_cscale[k];   // the moved sample, from its scaled row
        double h = g.h[k];
        if constexpr (ADAPT) h = h * lam;
        // truncated to [lower, upper): alpha = (lower - s) / h <= 0 < beta = (upper - s) / h.  The lower tail mass
        // pa = Phi(alpha), the upper tail mass qb = Phi(-beta), both accurate; a draw left of the median inverts
        // p = pa + u m, one right of it q = qb + (1 - u) m, so that neither tail is taken as 1 - (a number near 1)
        const double pa = kde_phi((g.lower[k] - s) / h);
        const double qb = kde_phi((s - g.upper[k]) / h);
        const double m = (0.5 - pa) + (0.5 - qb);
        const double uu = ((double)u[k] + 0.5) * 2.3283064365386963e-10;            // (0, 1)
        const double p = pa + uu * m;
        double z;
        if (p <= 0.5) {
          z = kde_phi_inv(p);
        } else {
          const double q = qb + ((double)(0xFFFFFFFFu - u[k]) + 0.5) * 2.3283064365386963e-10 * m;   // 1 - p
          z = -kde_phi_inv(q);
        }
        const double xd = s + h * z;
        float xf = (float)xd;
        // the evaluator's domain test in f64 on the float value: lower <= x < upper
        if (!((double)xf >= g.lower[k])) xf = g.bottom[k];
        if (!((double)xf < g.upper[k])) xf = g.top[k];
        x[k] = xf;
        if (g.has_cuts) ok = ok && !(xf > g.cut_hi[k] || xf < g.cut_lo[k]);
      }
      if (ok) break;
      // redrawn while outside the cuts (a new row and new coordinates); after 1024 attempts the host fails the call
      if (attempt == 1023) atomicAdd(exhausted, 1u);
    }
    float* o = out + e * (unsigned long long)(D + 1);
#pragma unroll
    for (int k = 0; k < D; k++) o[k] = x[k];
    o[D] = g.dataset;
  }
}

}  // namespace

// the in-domain rows of the last evaluation, in table order: idx[0 .. pos[npad - 1])
hipError_t sx_kde_compact(const float* rows, int rowlen, unsigned long long npad, unsigned* flag, unsigned* pos,
                          unsigned* idx, void* temp, size_t temp_bytes, hipStream_t s) {
  if (npad == 0) return hipSuccess;
  const unsigned grid = (unsigned)((npad + kKdeBlock - 1) / kKdeBlock);
  hipLaunchKernelGGL(kde_flag_kernel, dim3(grid), dim3(kKdeBlock), 0, s, rows, rowlen, npad, flag);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = sx_inclusive_sum_u32(flag, pos, (int)npad, temp, temp_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kde_scatter_kernel, dim3(grid), dim3(kKdeBlock), 0, s, flag, pos, npad, idx);
  return hipGetLastError();
}

hipError_t sx_kde_sample(int D, const float* rows, const double* lambda, const unsigned* idx, unsigned n,
                         const SxKdeSampleArgs& g, unsigned long long seed, unsigned long long nevents, float* out,
                         unsigned* exhausted, hipStream_t s) {
  if (nevents == 0) return hipSuccess;
  const unsigned long long b = (nevents + kKdeBlock - 1) / kKdeBlock;
  const dim3 grid((unsigned)(b < 4096 ? b : 4096));
  return kde_for_dim_adapt(D, lambda != nullptr, [&](auto dim, auto adapt) {
    hipLaunchKernelGGL((kde_sample_kernel<decltype(dim)::value, decltype(adapt)::value>), grid, dim3(kKdeBlock), 0, s,
                       rows, lambda, idx, n, g, seed, nevents, out, exhausted);
    return hipGetLastError();
  });
}

// cum[0 .. npad): the inclusive prefix sum of the live rows' multiplicities, in table order
hipError_t sx_kde_weighted_scan(const float* rows, int rowlen, unsigned long long npad, const unsigned* mult,
                                unsigned* flag, unsigned* cum, void* temp, size_t temp_bytes, hipStream_t s) {
  if (npad == 0) return hipSuccess;
  const unsigned grid = (unsigned)((npad + kKdeBlock - 1) / kKdeBlock);
  hipLaunchKernelGGL(kde_mflag_kernel, dim3(grid), dim3(kKdeBlock), 0, s, rows, rowlen, npad, mult, flag);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return sx_inclusive_sum_u32(flag, cum, (int)npad, temp, temp_bytes, s);
}

hipError_t sx_kde_sample_weighted(int D, const float* rows, const double* lambda, const unsigned* cum, unsigned total,
                                  unsigned long long npad, const SxKdeSampleArgs& g, unsigned long long seed,
                                  unsigned long long nevents, float* out, unsigned* exhausted, hipStream_t s) {
  if (nevents == 0) return hipSuccess;
  if (total == 0u || npad == 0 || npad > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const unsigned long long b = (nevents + kKdeBlock - 1) / kKdeBlock;
  const dim3 grid((unsigned)(b < 4096 ? b : 4096));
  return kde_for_dim_adapt(D, lambda != nullptr, [&](auto dim, auto adapt) {
    const KdePick pick{cum, (unsigned)npad};
    hipLaunchKernelGGL((kde_sample_kernel<decltype(dim)::value, decltype(adapt)::value, KdePick>), grid, dim3(kKdeBlock),
                       0, s, rows, lambda, (const unsigned*)nullptr, total, g, seed, nevents, out, exhausted, pick);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------ projection (sxmc_kde_project)
// The share of the PDF of the last evaluation in each of nbins equal bins of one observable: the kernel of an in-domain
// sample is a product of truncated Gaussians, the other observables integrate to their own truncation mass, and what is
// left is analytic, [Phi(t_j+1 - u) - Phi(t_j - u)] / [Phi(T - u) - Phi(-u)] per sample and bin.  Three launches:
//   kde_project_prep     one lane per sample row: u = c / sqrt(log2(e) / 2) and the reciprocal mass in f64 (0 for a row outside the
//                        domain) into scratch, once per sample instead of once per lane below; the in-domain count
//   kde_project_kernel   the pair kernel's shape: one lane per bin, the samples wave-uniform (scalar loads of u and the
//                        reciprocal mass), split across workgroups (blockIdx.y) so that a hundred bins fill the card
//   kde_project_combine  per bin the partials in split order, over the count
// f64 throughout, Phi through erfc as kde_prepass and kde_sample write it; no floating-point atomics.
namespace {

// ADAPT (an adaptive evaluator): rows of D + 2 floats, and per sample three scratch doubles -- u, the reciprocal mass
// taken at the sample's own bandwidth h lambda, and 1 / lambda, which scales every distance of the kernel below.
// WEIGHTED (`mult`: [npad] the rows' multiplicities): a live row's reciprocal mass times (double)m_i, and m_i counted.
template <bool ADAPT, class... MULT>
__global__ __launch_bounds__(kKdeBlock) void kde_project_prep_kernel(const float* __restrict__ rows,
                                                                     const SxKdeProjectArgs a,
                                                                     double* __restrict__ scratch,
                                                                     unsigned* __restrict__ count,
                                                                     const MULT... mult) {
  static_assert(kde_pack_is<KdeMult, MULT...>(), "the pack is empty or one KdeMult");
  constexpr bool WEIGHTED = sizeof...(MULT) == 1;
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  unsigned in = 0u;
  if (i < a.npad) {
    constexpr int kExtra = ADAPT ? 2 : 1;
    const float* row = rows + i * (unsigned long long)(a.D + kExtra);
    double u = 0.0, inv = 0.0, il = 1.0;
    if constexpr (ADAPT) il = 1.0 / a.lambda[i];
    if (row[a.D + kExtra - 1] > 0.0f) {
      in = 1u;
      u = (double)row[a.obs] / a.cunit;
      const double T = (a.upper - a.lower) / a.h;
      if constexpr (ADAPT) inv = 1.0 / (kde_phi((T - u) * il) - kde_phi(-u * il));
      else inv = 1.0 / (kde_phi(T - u) - kde_phi(-u));
      if constexpr (WEIGHTED) {
        in = kde_only(mult...).p[i];
        inv = inv * (double)in;
      }
    }
    if constexpr (ADAPT) {
      scratch[3ull * i] = u;
      scratch[3ull * i + 1ull] = inv;
      scratch[3ull * i + 2ull] = il;
    } else {
      scratch[2ull * i] = u;
      scratch[2ull * i + 1ull] = inv;
    }
  }
  // (every lane of the wave gets here)
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) in += __shfl_down(in, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && in != 0u) {
    __hip_atomic_fetch_add(count, in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// edge j of nbins equal bins as a distance from lower in bandwidths; the two ends are lower and upper themselves
__device__ __forceinline__ double kde_project_edge(const SxKdeProjectArgs& a, unsigned long long j) {
  if (j == 0ull) return 0.0;
  if (j >= (unsigned long long)a.nbins) return (a.upper - a.lower) / a.h;
  const double e = a.lower + (double)j * ((a.upper - a.lower) / (double)a.nbins);
  return (e - a.lower) / a.h;
}

template <bool ADAPT>
__global__ __launch_bounds__(SXMC_KDE_PROJ_LANES) void kde_project_kernel(const SxKdeProjectArgs a,
                                                                          const double* __restrict__ scratch,
                                                                          double* __restrict__ part) {
  const unsigned long long lane = (unsigned long long)blockIdx.x * SXMC_KDE_PROJ_LANES + threadIdx.x;
  // lanes past the last bin do the last bin's work (uniform trip count; their partial is never read)
  const unsigned long long j = lane < (unsigned long long)a.nbins ? lane : (unsigned long long)a.nbins - 1ull;
  const double t0 = kde_project_edge(a, j), t1 = kde_project_edge(a, j + 1ull);
  const unsigned long long r0 = (unsigned long long)blockIdx.y * a.rows_per_split;
  const unsigned long long r1 = r0 + a.rows_per_split < a.npad ? r0 + a.rows_per_split : a.npad;
  double sum = 0.0;
  for (unsigned long long i = r0; i < r1; i++) {
    constexpr unsigned long long kPer = ADAPT ? 3ull : 2ull;
    const double u = scratch[kPer * i];
    const double inv = scratch[kPer * i + 1ull];
    if (inv == 0.0) continue;   // (wave-uniform: a row outside the domain)
    if constexpr (ADAPT) {
      const double il = scratch[kPer * i + 2ull];
      sum += (kde_phi((t1 - u) * il) - kde_phi((t0 - u) * il)) * inv;
    } else {
      sum += (kde_phi(t1 - u) - kde_phi(t0 - u)) * inv;
    }
  }
  part[(unsigned long long)blockIdx.y * a.pitch + lane] = sum;
}

__global__ __launch_bounds__(kKdeBlock) void kde_project_combine_kernel(const SxKdeProjectArgs a,
                                                                        const double* __restrict__ part,
                                                                        const unsigned* __restrict__ count,
                                                                        double* __restrict__ prob) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (j >= (unsigned long long)a.nbins) return;
  double s = 0.0;
  for (unsigned k = 0; k < a.nsplit; k++) s += part[(unsigned long long)k * a.pitch + j];
  const unsigned n = *count;
  prob[j] = n == 0u ? 0.0 : s / (double)n;
}

}  // namespace

hipError_t sx_kde_project(const float* rows, const SxKdeProjectArgs& a, const unsigned* mult, double* scratch,
                          unsigned* count, double* d_prob, hipStream_t s) {
  if (a.nbins < 1 || a.npad == 0 || a.obs < 0 || a.obs >= a.D || a.rows_per_split == 0 ||
      (unsigned long long)a.nsplit * a.rows_per_split < a.npad || a.pitch % SXMC_KDE_PROJ_LANES != 0 ||
      a.pitch < (unsigned long long)a.nbins) {
    return hipErrorInvalidValue;
  }
  double* part = scratch + (a.lambda ? 3ull : 2ull) * a.npad;
  const dim3 prep((unsigned)((a.npad + kKdeBlock - 1) / kKdeBlock));
  const dim3 pb(kKdeBlock);
  if (mult) {
    const KdeMult m{mult};
    if (a.lambda) hipLaunchKernelGGL((kde_project_prep_kernel<true, KdeMult>), prep, pb, 0, s, rows, a, scratch, count, m);
    else hipLaunchKernelGGL((kde_project_prep_kernel<false, KdeMult>), prep, pb, 0, s, rows, a, scratch, count, m);
  } else if (a.lambda) {
    hipLaunchKernelGGL(kde_project_prep_kernel<true>, prep, pb, 0, s, rows, a, scratch, count);
  } else {
    hipLaunchKernelGGL(kde_project_prep_kernel<false>, prep, pb, 0, s, rows, a, scratch, count);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)(a.pitch / SXMC_KDE_PROJ_LANES), a.nsplit);
  if (a.lambda) hipLaunchKernelGGL(kde_project_kernel<true>, grid, dim3(SXMC_KDE_PROJ_LANES), 0, s, a, scratch, part);
  else hipLaunchKernelGGL(kde_project_kernel<false>, grid, dim3(SXMC_KDE_PROJ_LANES), 0, s, a, scratch, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kde_project_combine_kernel, dim3((unsigned)(((unsigned long long)a.nbins + kKdeBlock - 1) / kKdeBlock)),
                     dim3(kKdeBlock), 0, s, a, part, count, d_prob);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ pilot (sxmc_kde_create_adaptive)
// The fixed-bandwidth PDF at zero systematics taken at every table row, in f64, once per construction:
//   f_i = (1/n) sum_{j in S0} w_j prod_d phi((x_id - x_jd) / h_d) / h_d
// kde_project_kernel's shape: one lane per table row, the n in-domain samples wave-uniform (scalar loads of D
// coordinates and the weight), split across workgroups (blockIdx.y) by a rule that reads the sample count alone;
// kde_pilot_combine adds the splits in their order.  No floating-point atomics: the same bits on every device.
namespace {

template <int D>
__global__ __launch_bounds__(kKdeBlock) void kde_pilot_kernel(const SxKdePilotArgs a, const double* __restrict__ x,
                                                              const double* __restrict__ s0,
                                                              double* __restrict__ part) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;   // < pitch (whole blocks)
  double p[D];
#pragma unroll
  for (int k = 0; k < D; k++) p[k] = x[(unsigned long long)k * a.pitch + i];
  const unsigned long long j0 = (unsigned long long)blockIdx.y * a.per_split;
  const unsigned long long j1 = j0 + a.per_split < a.n ? j0 + a.per_split : a.n;
  double sum = 0.0;
  for (unsigned long long j = j0; j < j1; j++) {
    const double* r = s0 + j * (unsigned long long)(D + 1);
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < D; k++) {
      const double z = (p[k] - r[k]) / a.h[k];   // the difference first, then the bandwidth
      q = q + z * z;
    }
    sum += r[D] * exp(-0.5 * q);
  }
  part[(unsigned long long)blockIdx.y * a.pitch + i] = sum;
}

__global__ __launch_bounds__(kKdeBlock) void kde_pilot_combine_kernel(const SxKdePilotArgs a,
                                                                      const double* __restrict__ part,
                                                                      double* __restrict__ f) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= a.pitch) return;
  double s = 0.0;
  for (unsigned k = 0; k < a.nsplit; k++) s += part[(unsigned long long)k * a.pitch + i];
  f[i] = s * a.prefactor / (double)a.n;
}

// ... over weighted samples: the host hands m_j / mass_j as a row's weight and the multiplicities' total S1 stands in
// place of n (a sibling of the combine above; kde_pilot_kernel is the same for both)
__global__ __launch_bounds__(kKdeBlock) void kde_pilot_combine_weighted_kernel(const SxKdePilotArgs a,
                                                                               const double* __restrict__ part,
                                                                               double* __restrict__ f, double total) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= a.pitch) return;
  double s = 0.0;
  for (unsigned k = 0; k < a.nsplit; k++) s += part[(unsigned long long)k * a.pitch + i];
  f[i] = s * a.prefactor / total;
}

}  // namespace

hipError_t sx_kde_pilot(const SxKdePilotArgs& a, const double* x, const double* s0, double total, double* part,
                        double* f, hipStream_t s) {
  if (a.pitch == 0 || a.pitch % kKdeBlock != 0 || a.n == 0 || a.per_split == 0 ||
      (unsigned long long)a.nsplit * a.per_split < a.n) {
    return hipErrorInvalidValue;
  }
  const dim3 grid((unsigned)(a.pitch / kKdeBlock), a.nsplit);
  const hipError_t e = kde_for_dim(a.D, [&](auto dim) {
    hipLaunchKernelGGL(kde_pilot_kernel<decltype(dim)::value>, grid, dim3(kKdeBlock), 0, s, a, x, s0, part);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  const dim3 rows_grid((unsigned)(a.pitch / kKdeBlock));
  if (total > 0.0) hipLaunchKernelGGL(kde_pilot_combine_weighted_kernel, rows_grid, dim3(kKdeBlock), 0, s, a, part, f, total);
  else hipLaunchKernelGGL(kde_pilot_combine_kernel, rows_grid, dim3(kKdeBlock), 0, s, a, part, f);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ cross-validation (sxmc_kde_cv_scores)
// The leave-one-out log-likelihood of K candidate bandwidth vectors on m rows, one pass over the m^2 pairs in f64:
//   ln f_-i(h_c) = ln[ 1/(m-1) sum_{j != i} prod_d phi((x_id - x_jd) / h_cd) / (h_cd M_jd(h_c)) ]
//   kde_cv_weights  one lane per sample j: its K weights 1 / prod_d (h_cd M_jd), M through erfc as the prepass and the
//                   pilot write it, once per scan (0 for the padding candidates)
//   kde_cv_pairs    the pilot's shape: one lane per scored row i, the samples wave-uniform (scalar loads of the D
//                   coordinates and the KP weights), split across workgroups (blockIdx.y).  Per pair the D squared
//                   differences once; per candidate q = sum_d e_d g_cd with g = 1 / (2 h^2) (no division), one exp, one
//                   multiply-add into the candidate's own accumulator.  The pair j == i is left out by a select on the
//                   row index, never subtracted.
//   kde_cv_combine  per row and candidate the splits added in their order, times 1 / ((2 pi)^(D/2) (m - 1)), and the
//                   logarithm (-inf for a row without a neighbour in exp's range)
// The m logarithms of a candidate are added on the host in table order.  No floating-point atomics.
namespace {

__global__ __launch_bounds__(kKdeBlock) void kde_cv_weights_kernel(const SxKdeCvArgs a, double* __restrict__ s0,
                                                                   const double* __restrict__ cand) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (j >= a.m) return;
  double* row = s0 + j * (unsigned long long)(a.D + a.KP);
  const double* inv_h_sqrt2 = cand + (unsigned long long)a.KP * a.D;
  const double* prod_h = cand + 2ull * a.KP * a.D;
  for (int c = 0; c < a.KP; c++) {
    double w = 0.0;
    if (c < a.K) {
      double mass = 1.0;
      for (int d = 0; d < a.D; d++) {
        mass = mass * sxkde::truncation_mass(row[d], a.lower[d], a.upper[d], inv_h_sqrt2[c * a.D + d]);
      }
      w = 1.0 / (prod_h[c] * mass);
    }
    row[a.D + c] = w;
  }
}

template <int D, int KP>
__global__ __launch_bounds__(kKdeBlock) void kde_cv_pairs_kernel(const SxKdeCvArgs a, const double* __restrict__ x,
                                                                 const double* __restrict__ s0,
                                                                 const double* __restrict__ g,
                                                                 double* __restrict__ part) {
  const unsigned i = blockIdx.x * kKdeBlock + threadIdx.x;   // < pitch (whole blocks)
  double p[D];
#pragma unroll
  for (int k = 0; k < D; k++) p[k] = x[(unsigned long long)k * a.pitch + i];
  const unsigned j0 = blockIdx.y * a.per_split;
  const unsigned j1 = a.m - j0 > a.per_split ? j0 + a.per_split : a.m;   // (j0 < m: nsplit * per_split covers m tightly)
  double acc[KP];
#pragma unroll
  for (int c = 0; c < KP; c++) acc[c] = 0.0;
  for (unsigned j = j0; j < j1; j++) {
    const double* r = s0 + (unsigned long long)j * (D + KP);
    double e[D];
#pragma unroll
    for (int k = 0; k < D; k++) {
      const double z = p[k] - r[k];
      e[k] = z * z;
    }
    const bool other = j != i;
#pragma unroll
    for (int c = 0; c < KP; c++) {
      double q = e[0] * g[c * D];
#pragma unroll
      for (int k = 1; k < D; k++) q = __builtin_fma(e[k], g[c * D + k], q);
      const double t = r[D + c] * exp(-q);
      acc[c] += other ? t : 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < KP; c++) part[((unsigned long long)blockIdx.y * KP + c) * a.pitch + i] = acc[c];
}

__global__ __launch_bounds__(kKdeBlock) void kde_cv_combine_kernel(const SxKdeCvArgs a, const double* __restrict__ part,
                                                                   double* __restrict__ lnf) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  const unsigned c = blockIdx.y;   // < K
  if (i >= a.pitch) return;
  double s = 0.0;
  for (unsigned k = 0; k < a.nsplit; k++) s += part[((unsigned long long)k * a.KP + c) * a.pitch + i];
  lnf[(unsigned long long)c * a.pitch + i] = log(s * a.prefactor);
}

// the pair kernel of D observables and KP candidates (sx_kde_cv_padded: 1, 8, 16, 24 or 32)
template <int D>
hipError_t kde_cv_launch_pairs(const SxKdeCvArgs& a, const double* x, const double* s0, const double* cand, double* part,
                               hipStream_t s) {
  const dim3 grid((unsigned)(a.pitch / kKdeBlock), a.nsplit);
  const int nth = a.KP == 1 ? 1 : (a.KP >= 8 && a.KP % 8 == 0) ? a.KP / 8 + 1 : 0;   // of that list, from 1
  return kde_for_range<5>(nth, [&](auto n) {
    constexpr int KP = decltype(n)::value == 1 ? 1 : (decltype(n)::value - 1) * 8;
    hipLaunchKernelGGL((kde_cv_pairs_kernel<D, KP>), grid, dim3(kKdeBlock), 0, s, a, x, s0, cand, part);
    return hipGetLastError();
  });
}

}  // namespace

// the candidate counts the pair kernel is built for
int sx_kde_cv_padded(int K) { return K <= 1 ? 1 : (K + 7) / 8 * 8; }

hipError_t sx_kde_cv_scan(const SxKdeCvArgs& a, const double* x, double* s0, const double* cand, double* part,
                          double* lnf, hipStream_t s) {
  if (a.pitch == 0 || a.pitch % kKdeBlock != 0 || a.m < 2 || a.m > a.pitch || a.pitch > 0x7FFFFF00ull || a.K < 1 ||
      a.K > SXMC_KDE_CV_MAX || a.KP != sx_kde_cv_padded(a.K) || a.per_split == 0 || a.nsplit == 0 ||
      (unsigned long long)a.nsplit * a.per_split < a.m || (unsigned long long)(a.nsplit - 1) * a.per_split >= a.m) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(kde_cv_weights_kernel, dim3((a.m + kKdeBlock - 1) / kKdeBlock), dim3(kKdeBlock), 0, s, a, s0, cand);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = kde_for_dim(a.D, [&](auto dim) { return kde_cv_launch_pairs<decltype(dim)::value>(a, x, s0, cand, part, s); });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kde_cv_combine_kernel, dim3((unsigned)(a.pitch / kKdeBlock), (unsigned)a.K), dim3(kKdeBlock), 0, s, a,
                     part, lnf);
  return hipGetLastError();
}
