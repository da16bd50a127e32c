// project_kernels.hip -- the marginal of a histogram along one observable (sxmc_hist_project): what
// TH2D::ProjectionX / TH3D::ProjectionY ... do to the histogram plot_fit draws (plots.cpp:226-241), summed where the bins
// are instead of on a host copy of them.
//
// One pass over d_bins (row-major, last observable fastest): bin `flat` has index (flat / stride) % nb along the asked
// observable.  Integer atomics only, 64-bit totals, so the result does not depend on timing.
//   nb <= kProjLdsBins   every workgroup keeps a partial marginal of 64-bit counters in LDS (ds_add_u64) and hands the
//                        non-zero ones to the result at its end: one HBM atomic per workgroup and marginal bin
//   otherwise            one 64-bit HBM atomic per non-empty bin (an axis that long leaves few bins per counter: a
//                        1-D histogram none but the bin itself)
#include <hip/hip_runtime.h>

#include "sxmc_device.h"

namespace {

constexpr int kProjBlock = 256;
constexpr int kProjLdsBins = 2048;   // 16 KB of LDS per workgroup

template <bool LDS>
__global__ __launch_bounds__(kProjBlock) void hist_project_kernel(const unsigned* __restrict__ bins,
                                                                  unsigned long long total, unsigned stride, unsigned nb,
                                                                  unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[LDS ? kProjLdsBins : 1];
  if (LDS) {
    for (unsigned j = threadIdx.x; j < nb; j += kProjBlock) part[j] = 0ull;
    __syncthreads();
  }
  const unsigned long long step = (unsigned long long)gridDim.x * kProjBlock;
  for (unsigned long long flat = (unsigned long long)blockIdx.x * kProjBlock + threadIdx.x; flat < total; flat += step) {
    const unsigned c = bins[flat];
    if (c == 0u) continue;
    const unsigned j = ((unsigned)flat / stride) % nb;   // (total fits 31 bits: sxmc_hist_create refuses more)
    if (LDS) {
      atomicAdd(&part[j], (unsigned long long)c);
    } else {
      atomicAdd(&out[j], (unsigned long long)c);
    }
  }
  if (LDS) {
    __syncthreads();
    for (unsigned j = threadIdx.x; j < nb; j += kProjBlock) {
      const unsigned long long v = part[j];
      if (v != 0ull) atomicAdd(&out[j], v);
    }
  }
}

}  // namespace

// out[0 .. nb) must be zero; max_blocks: how many workgroups the device keeps resident
hipError_t sx_hist_project(const unsigned* d_bins, unsigned long long total, unsigned stride, unsigned nb,
                           unsigned long long* d_out, unsigned max_blocks, hipStream_t s) {
  if (total == 0 || nb == 0 || stride == 0) return hipErrorInvalidValue;
  const unsigned long long want = (total + kProjBlock - 1) / kProjBlock;
  const unsigned grid = (unsigned)(want < max_blocks ? want : (max_blocks ? max_blocks : 1));
  if (nb <= (unsigned)kProjLdsBins) {
    hipLaunchKernelGGL(hist_project_kernel<true>, dim3(grid), dim3(kProjBlock), 0, s, d_bins, total, stride, nb, d_out);
  } else {
    hipLaunchKernelGGL(hist_project_kernel<false>, dim3(grid), dim3(kProjBlock), 0, s, d_bins, total, stride, nb, d_out);
  }
  return hipGetLastError();
}
