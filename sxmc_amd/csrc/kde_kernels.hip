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
#include <hip/hip_runtime.h>

#include "sxmc_device.h"

#include "fill_kernels.inc.h"

#pragma clang fp contract(off)

namespace {

using namespace sxfill;

constexpr int kKdeTile = SXMC_KDE_TILE;   // samples per f32 partial sum (the sample rows are padded to a multiple)
constexpr int kKdeBlock = 256;

template <int NSLOT>
__global__ __launch_bounds__(kKdeBlock) void kde_prepass_kernel(const SxSignalDesc d, const SxKdeArgs a) {
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
    cnt += in ? 1u : 0u;
    if (i < a.npad) {
      double mass = 1.0;
      float* row = a.rows + i * (unsigned long long)(d.nobs + 1);
#pragma unroll
      for (int k = 0; k < D; k++) {
        if (k >= d.nobs) continue;
        const double x = in ? f[k][q] : a.lower[k];
        // Phi(z) = erfc(-z / sqrt 2) / 2 with z = (edge - x) / h
        mass = mass * (0.5 * (erfc((x - a.upper[k]) * a.inv_h_sqrt2[k]) - erfc((x - a.lower[k]) * a.inv_h_sqrt2[k])));
        row[k] = in ? (float)((x - a.lower[k]) * a.cscale[k]) : 0.0f;
      }
      row[d.nobs] = in ? (float)(1.0 / mass) : 0.0f;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
  if (lane == 0 && cnt != 0u) __hip_atomic_fetch_add(a.norm, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per point; every lane of the grid runs the full trip count (points are padded with zeros), so the sample
// rows are read at wave-uniform addresses: scalar loads, SGPR operands of the vector instructions.
template <int D>
__global__ __launch_bounds__(kKdeBlock) void kde_pairs_kernel(const float* __restrict__ pts, unsigned long long pitch,
                                                              const float* __restrict__ rows, unsigned tiles_per_split,
                                                              unsigned ntiles, double* __restrict__ part) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  float p[D];
#pragma unroll
  for (int k = 0; k < D; k++) p[k] = pts[(unsigned long long)k * pitch + i];
  const unsigned t0 = blockIdx.y * tiles_per_split;
  const unsigned t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  double sum = 0.0;
  for (unsigned t = t0; t < t1; t++) {
    const float* s = rows + (unsigned long long)t * kKdeTile * (D + 1);
    float acc = 0.0f;
#pragma unroll 16
    for (int j = 0; j < kKdeTile; j++) {
      const float* r = s + j * (D + 1);
      const float a0 = p[0] - r[0];
      float q = a0 * a0;
#pragma unroll
      for (int k = 1; k < D; k++) {
        const float ak = p[k] - r[k];
        q = __builtin_fmaf(ak, ak, q);
      }
      acc = __builtin_fmaf(r[D], __builtin_amdgcn_exp2f(-q), acc);
    }
    sum += (double)acc;
  }
  part[(unsigned long long)blockIdx.y * pitch + i] = sum;
}

__global__ __launch_bounds__(kKdeBlock) void kde_combine_kernel(const double* __restrict__ part, unsigned long long pitch,
                                                                int nsplit, unsigned long long npoints,
                                                                const int* __restrict__ codes,
                                                                const unsigned* __restrict__ norm, double prefactor,
                                                                float* __restrict__ out, long stride) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kKdeBlock + threadIdx.x;
  if (i >= npoints) return;
  const int code = codes[i];
  float v;
  if (code == -2) {
    v = 0.0f;                              // in the domain, another data set (pdfz.cpp:423-434)
  } else if (code < 0) {
    v = __int_as_float(0x7fc00000);        // outside the domain
  } else {
    double s = 0.0;
    for (int k = 0; k < nsplit; k++) s += part[(unsigned long long)k * pitch + i];
    const unsigned n = *norm;
    v = n == 0u ? __int_as_float(0x7fc00000) : (float)(s * prefactor / (double)n);
  }
  out[stride * (long)i] = v;
}

}  // namespace

hipError_t sx_kde_prepass(const SxSignalDesc& d, const SxKdeArgs& a, hipStream_t s) {
  const unsigned long long nvec = a.npad / SXMC_VEC;
  const unsigned grid = (unsigned)((nvec + kKdeBlock - 1) / kKdeBlock);
  if (grid == 0) return hipSuccess;
  switch (d.nslot) {
#define SX_KDE_CASE(N) \
  case N: hipLaunchKernelGGL(kde_prepass_kernel<N>, dim3(grid), dim3(kKdeBlock), 0, s, d, a); break;
    SX_KDE_CASE(1) SX_KDE_CASE(2) SX_KDE_CASE(3) SX_KDE_CASE(4) SX_KDE_CASE(5) SX_KDE_CASE(6) SX_KDE_CASE(7)
#undef SX_KDE_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t sx_kde_pairs(int D, const float* pts, unsigned long long pitch, const float* rows, unsigned tiles_per_split,
                        unsigned ntiles, int nsplit, double* part, hipStream_t s) {
  const dim3 grid((unsigned)(pitch / kKdeBlock), (unsigned)nsplit);
  switch (D) {
    case 1: hipLaunchKernelGGL(kde_pairs_kernel<1>, grid, dim3(kKdeBlock), 0, s, pts, pitch, rows, tiles_per_split, ntiles, part); break;
    case 2: hipLaunchKernelGGL(kde_pairs_kernel<2>, grid, dim3(kKdeBlock), 0, s, pts, pitch, rows, tiles_per_split, ntiles, part); break;
    case 3: hipLaunchKernelGGL(kde_pairs_kernel<3>, grid, dim3(kKdeBlock), 0, s, pts, pitch, rows, tiles_per_split, ntiles, part); break;
    case 4: hipLaunchKernelGGL(kde_pairs_kernel<4>, grid, dim3(kKdeBlock), 0, s, pts, pitch, rows, tiles_per_split, ntiles, part); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t sx_kde_combine(const double* part, unsigned long long pitch, int nsplit, unsigned long long npoints,
                          const int* codes, const unsigned* norm, double prefactor, float* out, long stride,
                          hipStream_t s) {
  if (npoints == 0) return hipSuccess;
  const unsigned grid = (unsigned)((npoints + kKdeBlock - 1) / kKdeBlock);
  hipLaunchKernelGGL(kde_combine_kernel, dim3(grid), dim3(kKdeBlock), 0, s, part, pitch, nsplit, npoints, codes, norm,
                     prefactor, out, stride);
  return hipGetLastError();
}
