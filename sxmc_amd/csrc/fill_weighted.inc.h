// fill_weighted.inc.h -- the WEIGHTED histogram fill of libsxmc_hip.so, written for gfx950 only: every row of the table
// counts with an integer multiplicity m_i (sxmc_hist_set_sample_multiplicities, include/sxmc_hip.h) where the fills of
// fill_kernels.inc.h count it once.  Included by pdfz_kernels.hip behind fill_kernels.inc.h, whose helpers it uses and
// whose kernels it leaves alone; not compiled at run time (a weighted launch class never asks for a specialisation).
//
// The law: bins[b] = sum of m_i over the rows the reference's arithmetic (bin_samples, src/pdfz.cpp:349-408) puts into
// bin b; norm = sum of m_i over the rows that pass the domain test, the in-domain row whose index comes out one past
// the end included.  Nothing else about an evaluation changes: counts are integers, integer atomics commute, and the
// host caps sum m_i at 2^32 - 1, so no partial sum -- a lane's, a workgroup's LDS word, a bin -- can overflow.
//
// The table is the one the rows form streams (kFormRows): the float columns as they are, plus ONE more column of
// `unsigned`, one word per row, padded with 0 to the columns' pitch -- the descriptor's `pre` (a weighted class has no
// pre-binned column, so the field is free).  20 bytes per row and observable-free slot where the rows form streams 16.
#pragma once

#include "sxmc_device_types.h"

#pragma clang fp contract(off)

namespace sxfill {

typedef unsigned vuint4w __attribute__((ext_vector_type(4)));  // the multiplicities of one 4-sample unit: one 16-byte load

template <int NSLOT>
struct WeightedColumns {
  vfloat4 v[NSLOT];
  vuint4w m;
};

// Issue order pinned as in load_columns: the float columns in slot order, then the multiplicities -- the prologue's and the
// steady state's loads are then the same sequence and the loop header waits by count (vmcnt(#loads)), not for a drain.
template <int NSLOT>
__device__ __forceinline__ void load_weighted_columns(WeightedColumns<NSLOT>& c, const gptr<const vfloat4> (&col)[NSLOT],
                                                      gptr<const vuint4w> mcol, unsigned long long v) {
#pragma unroll
  for (int k = 0; k < NSLOT; k++) {
    c.v[k] = stream_load<vfloat4>(&col[k][v]);
    __builtin_amdgcn_sched_barrier(0);
  }
  c.m = stream_load<vuint4w>(&mcol[v]);
  __builtin_amdgcn_sched_barrier(0);
}

// fill_body's shape (partition, LDS layout, trash words, one unit in flight per lane, clamped unconditional loads: see
// there), over the rows form only, histogram in LDS or beyond it (dense global atomics: a group with a weighted member
// evaluates in the dense flavour, sxmc_launch_plan.cpp build_sparse_descs).
template <int NOBS, int NSLOT, bool LDS_HIST, typename PROG>
__device__ __forceinline__ void fill_weighted_body(const SxSignalDesc* __restrict__ descs,
                                                   const SxSegment* __restrict__ segs,
                                                   const unsigned* __restrict__ blk_off, unsigned hist_words) {
  extern __shared__ unsigned lds[];
  const unsigned tid = threadIdx.x;
  const unsigned nthreads = blockDim.x;
  const unsigned lane = tid & (kWave - 1);

  unsigned* s_norm = lds;
  unsigned* hist = lds + 4;
  const unsigned trash = hist_words + lane;

  bool lds_clean = false;
  const unsigned seg_end = blk_off[blockIdx.x + 1];

  for (unsigned si = blk_off[blockIdx.x]; si < seg_end; ++si) {
    const SxSegment& sg = segs[si];
    const SxSignalDesc& d = descs[sg.sig];
    const unsigned long long v0 = sg.v0;
    const unsigned long long v1 = sg.v1;
    const unsigned long long step = sg.step;

    const unsigned B = (unsigned)d.total_nbins;
    gptr<unsigned> gbins = to_global(d.bins);

    // ---- the member's systematics, requested first (loads return in order: see fill_body)
    const int nsyst = d.nsyst;
    unsigned opword = 0u;
    double coef = 0.0;
    double craw[PROG::ncoef > 0 ? PROG::ncoef : 1];
    if constexpr (PROG::dynamic) {
      if ((int)lane < nsyst) opword = pack_opword(d.syst[lane]);
      if ((int)lane < d.ncoef) coef = to_global(d.params)[(long)d.coef_par[lane] * d.param_stride];
    } else {
#pragma unroll
      for (int q = 0; q < PROG::ncoef; q++) craw[q] = to_global(d.params)[(long)d.coef_par[q] * d.param_stride];
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- the first unit's columns and multiplicities, before anything else is set up
    gptr<const vfloat4> col[NSLOT];
#pragma unroll
    for (int k = 0; k < NSLOT; k++) {
      col[k] = to_global(reinterpret_cast<const vfloat4*>(d.cols + (unsigned long long)d.slot_col[k] * d.col_pitch));
    }
    gptr<const vuint4w> mcol = to_global(reinterpret_cast<const vuint4w*>(d.pre));
    const unsigned long long vlast = v1 - 1;
    const unsigned long long vfirst = v0 + tid;
    WeightedColumns<NSLOT> bufA;
    load_weighted_columns<NSLOT>(bufA, col, mcol, vfirst < v1 ? vfirst : vlast);

    if (!lds_clean) {
      if (LDS_HIST) {
        for (unsigned b = tid; b < hist_words; b += nthreads) hist[b] = 0u;
      }
      if (tid == 0) *s_norm = 0u;
      __syncthreads();
    }

    // ---- wave-uniform geometry into scalar registers
    double lo[NOBS], hi[NOBS], sc[NOBS];
    int st[NOBS];
#pragma unroll
    for (int k = 0; k < NOBS; k++) {
      lo[k] = d.lower[k];
      hi[k] = d.upper[k];
      sc[k] = d.scale[k];
      st[k] = d.bin_stride[k];
    }

    unsigned cnt = 0;   // sum of m over this lane's in-domain rows

    auto stage = [&](WeightedColumns<NSLOT>& buf, const unsigned long long vc) {
      double f[NSLOT][SXMC_VEC];
#pragma unroll
      for (int k = 0; k < NSLOT; k++) {
        f[k][0] = (double)buf.v[k].x;
        f[k][1] = (double)buf.v[k].y;
        f[k][2] = (double)buf.v[k].z;
        f[k][3] = (double)buf.v[k].w;
      }
      unsigned mq[SXMC_VEC] = {buf.m.x, buf.m.y, buf.m.z, buf.m.w};
      // Pin every widening and the four multiplicities BEFORE the buffer is re-loaded (see fill_body: a value that stays
      // live in the buffer's registers across the reload makes the reload land in fresh ones, behind a full wait).
#pragma unroll
      for (int k = 0; k < NSLOT; k++) {
#pragma unroll
        for (int q = 0; q < SXMC_VEC; q++) asm volatile("" : "+v"(f[k][q]));
      }
#pragma unroll
      for (int q = 0; q < SXMC_VEC; q++) asm volatile("" : "+v"(mq[q]));
      const unsigned long long vl = vc + step;
      load_weighted_columns<NSLOT>(buf, col, mcol, vl < v1 ? vl : vlast);

      if constexpr (PROG::dynamic) {
        for (int s = 0; s < nsyst; s++) {
          apply_op<NSLOT>(f, (unsigned)__builtin_amdgcn_readlane((int)opword, s), coef);
        }
      } else {
        run_static<NSLOT>(f, craw, PROG{}, typename MakeISeq<PROG::n>::type{});
      }

      // lanes past the end of the slice hold clamped duplicates: they fail, and their m goes to the trash word
      const unsigned dead = (vc < v1) ? 0u : 1u;
#pragma unroll
      for (int q = 0; q < SXMC_VEC; q++) {
        // pdfz.cpp:388-398, as fill_body forms it: NaN fails every test
        unsigned bad = dead;
        int bin = 0;
#pragma unroll
        for (int k = 0; k < NOBS; k++) {
          const double x = f[k][q];
          bad += !(x >= lo[k]) ? 1u : 0u;
          bad += !(x < hi[k]) ? 1u : 0u;
          const int idx = (int)((x - lo[k]) * sc[k]);
          if (LDS_HIST) {
            bin = (k == NOBS - 1) ? bin + idx : __mul24(idx, st[k]) + bin;
          } else {
            bin += idx * st[k];
          }
        }
        cnt += (bad == 0u) ? mq[q] : 0u;
        // in domain but index out of range (the one-past-the-end case) counts in the norm and is not histogrammed
        const bool store = (bad == 0u) && ((unsigned)bin < B);
        if (LDS_HIST) {
          const unsigned slot = store ? (unsigned)bin : trash;
          __hip_atomic_fetch_add(&hist[slot], mq[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (store && mq[q] != 0u) {   // (a row of multiplicity 0 sends no atomic to HBM)
          __hip_atomic_fetch_add(&gbins[(unsigned)bin], mq[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    };

    // wave-uniform trip count: every lane runs the same number of stages
    unsigned long long v = vfirst;
    const unsigned long long niter = (v1 - v0 + step - 1) / step;
    for (unsigned long long it = 0; it < niter; ++it, v += step) stage(bufA, v);

    // ---- in-domain total: lane registers -> wave -> workgroup -> one global atomic
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
    if (lane == 0 && cnt != 0u) {
      __hip_atomic_fetch_add(s_norm, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();

    // ---- flush: only non-zero bins reach HBM; cleared afterwards if another member follows
    if (LDS_HIST) {
#pragma unroll 4
      for (unsigned b = tid; b < B; b += nthreads) {
        const unsigned c = hist[b];
        if (c != 0u) __hip_atomic_fetch_add(&gbins[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (si + 1u < seg_end) {
        __syncthreads();
        for (unsigned b = tid; b < B; b += nthreads) hist[b] = 0u;
      }
    }
    if (tid == 0) {
      const unsigned c = *s_norm;
      if (c != 0u) __hip_atomic_fetch_add(to_global(d.norm), c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *s_norm = 0u;
    }
    __syncthreads();
    lds_clean = true;
  }
}

template <int NOBS, int NSLOT, bool LDS_HIST, typename PROG>
__global__ __launch_bounds__(1024) void fill_weighted_kernel(const SxSignalDesc* __restrict__ descs,
                                                             const SxSegment* __restrict__ segs,
                                                             const unsigned* __restrict__ blk_off, unsigned hist_words) {
  fill_weighted_body<NOBS, NSLOT, LDS_HIST, PROG>(descs, segs, blk_off, hist_words);
}

// Shape-agnostic weighted fill (any nobs / nslot up to SXMC_MAX_NFIELDS): one row per lane per iteration, fields in a
// dynamically indexed array -- fill_kernel_generic's loop (pdfz_kernels.hip) with the row's multiplicity in the place of 1.
template <bool LDS_HIST>
__global__ __launch_bounds__(1024) void fill_weighted_kernel_generic(const SxSignalDesc* __restrict__ descs,
                                                                     const SxSegment* __restrict__ segs,
                                                                     const unsigned* __restrict__ blk_off,
                                                                     unsigned hist_words) {
  extern __shared__ unsigned lds[];
  const unsigned tid = threadIdx.x;
  const unsigned nthreads = blockDim.x;
  unsigned* s_norm = lds;
  unsigned* hist = lds + 4;

  bool lds_clean = false;
  const unsigned seg_end = blk_off[blockIdx.x + 1];

  for (unsigned si = blk_off[blockIdx.x]; si < seg_end; ++si) {
    const SxSegment& sg = segs[si];
    const SxSignalDesc& d = descs[sg.sig];
    const unsigned long long v0 = sg.v0;
    const unsigned long long v1 = sg.v1;
    const unsigned long long step = sg.step;
    const unsigned B = (unsigned)d.total_nbins;
    gptr<unsigned> gbins = to_global(d.bins);
    gptr<const unsigned> mcol = to_global(reinterpret_cast<const unsigned*>(d.pre));
    if (!lds_clean) {
      if (LDS_HIST) {
        for (unsigned b = tid; b < hist_words; b += nthreads) hist[b] = 0u;
      }
      if (tid == 0) *s_norm = 0u;
      __syncthreads();
    }
    const int nobs = d.nobs, nslot = d.nslot, nsyst = d.nsyst;
    gptr<const double> params = to_global(d.params);
    const int pstride = d.param_stride;
    unsigned cnt = 0;
    // v counts 4-sample units; a workgroup covers units [c, c + nthreads) for c = v0, v0 + step, ...
    for (unsigned long long c = v0; c < v1; c += step)
    for (unsigned long long i = c * SXMC_VEC + tid;
         i < (c + nthreads < v1 ? c + nthreads : v1) * SXMC_VEC; i += nthreads) {
      const unsigned m = mcol[i];   // (the padding rows of the last unit: 0 here, NaN in the float columns)
      double f[SXMC_MAX_NFIELDS];
      for (int k = 0; k < nslot; k++) {
        f[k] = (double)to_global(d.cols)[(unsigned long long)d.slot_col[k] * d.col_pitch + i];
      }
      for (int s = 0; s < nsyst; s++) {
        const SxSystOp& op = d.syst[s];
        double x = f[op.obs_slot];
        double p = 0.0, pw = 1.0, pl = 0.0;
        for (int t = 0; t < op.npars; t++) {
          p = p + params[(long)op.pars[t] * pstride] * pw;
          pow_step(pw, pl, x);
        }
        switch (op.type) {
          case SXMC_SYST_SHIFT: x = x + p; break;
          case SXMC_SYST_SCALE: x = x * (1 + p); break;
          case SXMC_SYST_CTSCALE: x = 1 + (x - 1) * (1 + p); break;
          case SXMC_SYST_RESOLUTION_SCALE: x = x + (p * (x - f[op.extra_slot])); break;
          default: break;
        }
        f[op.obs_slot] = x;
      }
      bool ok = true;
      int bin = 0;
      for (int k = 0; k < nobs && ok; k++) {
        const double x = f[k];
        ok = (x >= d.lower[k]) && (x < d.upper[k]);
        if (ok) bin += (int)((x - d.lower[k]) * d.scale[k]) * d.bin_stride[k];
      }
      if (ok && m != 0u) {
        cnt += m;
        if ((unsigned)bin < B) {
          if (LDS_HIST) {
            __hip_atomic_fetch_add(&hist[bin], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            __hip_atomic_fetch_add(&gbins[bin], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
    if ((tid & (kWave - 1)) == 0 && cnt != 0u) {
      __hip_atomic_fetch_add(s_norm, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (LDS_HIST) {
      for (unsigned b = tid; b < B; b += nthreads) {
        const unsigned c = hist[b];
        if (c != 0u) {
          __hip_atomic_fetch_add(&gbins[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          hist[b] = 0u;
        }
      }
    }
    if (tid == 0) {
      const unsigned c = *s_norm;
      if (c != 0u) __hip_atomic_fetch_add(to_global(d.norm), c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *s_norm = 0u;
    }
    __syncthreads();
    lds_clean = true;
  }
}

}  // namespace sxfill
