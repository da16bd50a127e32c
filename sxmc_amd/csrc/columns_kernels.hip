// columns_kernels.hip -- gfx950 kernel for the event sum of a MIXED fit (wave64 only): nll_event_chunks
// (nll_kernels.hip; the reference's src/nll_kernels.cpp:89-116) over a lookup table whose columns are either
// materialised floats -- written by somebody else, a kernel-density evaluator for instance -- or histogram look-ups done
// in place, eval_pdf (src/pdfz.cpp:411-436) without the table in between.
//
// THE CONTRACT IS BIT EQUALITY with nll_event_chunks_kernel over the fully materialised table, launched with the same
// grid and block: lane t sums events t, t + grid * block, ... in index order; per event the terms are added in signal
// order, s = s + coef_j * (double)(isnan(v) ? 0 : v) with coef_j = pars[source_id[j]] * nexpected[j] *
// (float)(1.0 * norms[j] / n_mc[j]) evaluated left to right; log(s) is added only when s > 0; a NaN lane sum is not
// stored; no events: zeros.  A histogram column's v is eval_pdf_kernel's pdf_value (pdfz_kernels.hip): -2 -> 0, another
// negative -> NaN, else (float)((double)bins[rb] / ((double)norm * bin_volume)) with the member's own norm slot.  No
// contraction (the flag and the pragma below), as in nll_kernels.hip and pdfz_kernels.hip.
//
// How: like the kernels it restates it is a chain of dependent gathers (read_bins -> bins) on the reference's 64
// workgroups, so the columns' pointers and factors are staged in LDS once per workgroup, the first-level loads of
// sixteen columns are issued together (a dense column's float travels as its bits through the same load), then their
// gathers together (a dense column, or a row outside a member, reads a word that is always there and drops it: no
// branches between the loads), and the NEXT event's first sixteen are requested before this event's divisions and
// logarithm.
#include <hip/hip_runtime.h>

#include "sxmc_device.h"

#pragma clang fp contract(off)

namespace {

template <typename T>
using gptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ gptr<T> to_global(T* p) {
  return (gptr<T>)p;
}

struct ColumnRec {
  const int* first;        // histogram: the events' bins (read_bins); dense: the column itself, a float's bits per event
  const unsigned* second;  // histogram: the counters; dense: unused
  double bin_norm;         // histogram: (double)norm * bin_volume
  double coef;             // pars[sid] * nexpected * eff, the event-independent factor of nll_kernels.cpp:107
  int hist;
  int pad;
};

__global__ __launch_bounds__(256) void nll_columns_kernel(const SxSignalDesc* __restrict__ descs,
                                                          const int* __restrict__ member_of, const float* __restrict__ lut,
                                                          const double* __restrict__ pars, size_t ne, size_t ns,
                                                          const double* __restrict__ nexpected,
                                                          const unsigned* __restrict__ n_mc,
                                                          const short* __restrict__ source_id,
                                                          const unsigned* __restrict__ norms, double* sums) {
  extern __shared__ double s_raw[];
  ColumnRec* s_col = reinterpret_cast<ColumnRec*>(s_raw);   // [ns]
  const size_t offset = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (ne == 0 || ns == 0) {   // uniform
    sums[offset] = 0.0;
    return;
  }
  for (size_t j = threadIdx.x; j < ns; j += blockDim.x) {
    const float eff = (float)(1.0 * norms[j] / n_mc[j]);             // nll_kernels.cpp:105
    ColumnRec r;
    r.coef = pars[source_id[j]] * nexpected[j] * eff;                // left to right, :107
    const int m = member_of[j];
    if (m >= 0) {
      const SxSignalDesc& d = descs[m];
      r.first = d.read_bins;
      r.second = d.bins;
      r.bin_norm = (double)(*to_global((const unsigned*)d.norm)) * d.bin_volume;
      r.hist = 1;
    } else {
      r.first = reinterpret_cast<const int*>(lut + j * ne);
      r.second = norms;
      r.bin_norm = 1.0;
      r.hist = 0;
    }
    r.pad = 0;
    s_col[j] = r;
  }
  __syncthreads();

  constexpr int U = 16;
  // first level, event i, columns j0 .. j0 + U (indices past the last column repeat it, an event past the last one is
  // clamped: every load is issued on every path)
  auto request = [&](size_t i, size_t j0, int* w) {
    const size_t ic = i < ne ? i : ne - 1;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t j = j0 + (size_t)u < ns ? j0 + (size_t)u : ns - 1;
      w[u] = to_global(s_col[j].first)[ic];
    }
  };
  double sum = 0;
  int nxt[U];
  request(offset, 0, nxt);
  for (size_t i = offset; i < ne; i += stride) {
    double s = 0;
    int w[U];
#pragma unroll
    for (int u = 0; u < U; u++) w[u] = nxt[u];
    for (size_t j0 = 0; j0 < ns; j0 += U) {
      if (j0 > 0) request(i, j0, w);
      // second level: the counters of the histogram columns (everything else reads norms[0], which is always there)
      unsigned c[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t j = j0 + (size_t)u < ns ? j0 + (size_t)u : ns - 1;
        const bool look = s_col[j].hist != 0 && w[u] >= 0;
        const unsigned* p = look ? s_col[j].second + w[u] : norms;
        c[u] = *to_global(p);
      }
      if (j0 + U >= ns) request(i + stride, 0, nxt);   // (past the last event: a clamped, unused read)
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (j0 + (size_t)u < ns) {
          const ColumnRec& r = s_col[j0 + u];
          float v;
          if (r.hist) {
            // pdf_value (pdfz.cpp:423-434)
            v = w[u] == -2 ? 0.0f : w[u] < 0 ? __int_as_float(0x7fc00000) : (float)((double)c[u] / r.bin_norm);
          } else {
            v = __int_as_float(w[u]);
          }
          s = s + r.coef * (double)(!isnan(v) ? v : 0.0f);   // NaN: empty histogram
        }
      }
    }
    if (s > 0) sum += log(s);
  }
  if (!isnan(sum)) sums[offset] = sum;
}

}  // namespace

hipError_t sx_launch_nll_columns(const SxSignalDesc* d_descs, const int* d_member_of, int nsignals,
                                            const float* lut, unsigned long long ne, const double* pars,
                                            const double* nexpected, const unsigned* n_mc, const short* source_id,
                                            const unsigned* norms, double* sums, int grid, int block, hipStream_t s) {
  hipLaunchKernelGGL(nll_columns_kernel, dim3(grid), dim3(block), (size_t)nsignals * sizeof(ColumnRec), s, d_descs,
                     d_member_of, lut, pars, (size_t)ne, (size_t)nsignals, nexpected, n_mc, source_id, norms, sums);
  return hipGetLastError();
}
