// pdfz_kernels.hip -- gfx950 kernels for the pdfz::EvalHist half of the NLL evaluation:
// zero, histogram fill with per-sample systematics, PDF lookup, pre-binning and the row/column
// transposes, with the registry of the fill programs built in and their launchers.  Written for
// CDNA4 only (wave64, 160 KiB LDS per CU, 256 CUs); no other target is supported.
// The fill kernels' bodies are fill_kernels.inc.h (also compiled at run time, sxmc_rtc.cpp); the end
// of a Metropolis step -- event sum, finish_nll_jump_pick_combo, clearing, in all its forms, with
// its launchers -- is step_end_kernels.inc.h, part of this translation unit: the fused step's
// kernels below are fills that go on as step-end roles (fill_step_body).
//
// What is computed is fixed by the reference (file:line relative to /root/reference):
//   zero_hist    src/pdfz.cpp:334-346
//   bin_samples  src/pdfz.cpp:349-408  (+ apply_systematic 306-331)
//   eval_pdf     src/pdfz.cpp:411-436
// How it is computed is not: the samples are stored column-major and read with one 16-byte
// load per lane per column, each workgroup owns a contiguous slice of the concatenated sample
// index space of ALL signals, accumulates into an LDS-private uint32 histogram with ds_add_u32
// and flushes only its non-zero bins with one global atomic each; in-domain counts are kept in
// a register per lane and reduced once per workgroup.
//
// Exactness: double arithmetic is IEEE add/sub/mul with NO contraction (compile flag
// -ffp-contract=off plus the pragma below), in the reference's operation order, so bin
// indices are bit-identical to the reference CPU loop.  x^i of the polynomial systematics is
// rounded once (pow_step in fill_kernels.inc.h), like libm's pow for these exponents.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "nll_device.h"

#include "fill_kernels.inc.h"

#pragma clang fp contract(off)

#include "step_end_kernels.inc.h"

namespace {

using namespace sxfill;


// ------------------------------------------------------------------------------------ zero
// bins <- 0, norm <- 0 for every member (blockIdx.y = member).
__global__ __launch_bounds__(256) void zero_kernel(const SxSignalDesc* __restrict__ descs, unsigned* ticket) {
  const SxSignalDesc& d = descs[blockIdx.y];
  clear_piece(d.bins, (unsigned)d.total_nbins, blockIdx.x, gridDim.x, blockDim.x);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) *d.norm = 0u;
    if (threadIdx.x == 0 && blockIdx.y == 0 && ticket) *ticket = 0u;  // arrival counter of the fused step end
  }
}


// Shape-agnostic fallback (any nobs/nslot up to SXMC_MAX_NFIELDS): one sample per lane per
// iteration, fields in a dynamically indexed array.  Correctness path for shapes without a
// specialization; same arithmetic.  WEIGHTED: every row counts with its multiplicity (the descriptor's `pre`, one word
// per row: fill_body's law), dense histograms only.
template <bool LDS_HIST, bool WEIGHTED = false>
__global__ __launch_bounds__(1024) void fill_kernel_generic(const SxSignalDesc* __restrict__ descs,
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
    const bool sparse = !WEIGHTED && !LDS_HIST && d.sparse_table != nullptr;
    const unsigned B = sparse ? (unsigned)d.sparse_real_nbins : (unsigned)d.total_nbins;
    gptr<unsigned> gbins = to_global(d.bins);
    gptr<const unsigned> mcol = to_global(reinterpret_cast<const unsigned*>(d.pre));
    if (!lds_clean) {
      // whole LDS histogram (sized for the largest member), once per workgroup
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
      unsigned m = 1u;
      if constexpr (WEIGHTED) m = mcol[i];   // (the padding rows of the last unit: 0 here, NaN in the float columns)
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
      if (ok && (!WEIGHTED || m != 0u)) {
        cnt += m;
        if ((unsigned)bin < B) {
          if (LDS_HIST) {
            __hip_atomic_fetch_add(&hist[bin], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else if (sparse) {
            sparse_count(d, gbins, (unsigned)bin);
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

// ------------------------------------------------------------------------------------ eval
__device__ __forceinline__ float pdf_value(int rb, gptr<const unsigned> bins, double bin_norm) {
  // pdfz.cpp:423-434: -2 -> 0, other negatives -> NaN, else (float)(bins / (norm * volume))
  if (rb == -2) return 0.0f;
  if (rb < 0) return __int_as_float(0x7fc00000);
  return (float)((double)bins[rb] / bin_norm);
}

__global__ __launch_bounds__(256) void eval_pdf_kernel(const SxSignalDesc* __restrict__ descs) {
  const SxSignalDesc& d = descs[blockIdx.y];
  if (d.read_bins == nullptr) return;
  gptr<const int> rbs = to_global(d.read_bins);
  gptr<const unsigned> bins = to_global((const unsigned*)d.bins);
  const unsigned long long n = d.npoints;
  const double bin_norm = (double)(*to_global((const unsigned*)d.norm)) * d.bin_volume;
  gptr<float> out = to_global(d.pdf_out);
  const long stride = d.pdf_stride;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    out[stride * (long)i] = pdf_value(rbs[i], bins, bin_norm);
  }
}

// THE WHOLE STEP IN ONE LAUNCH: a fill whose grid carries the cooperative step end's roles behind the fill's workgroups
// (fill_step_body, step_end_kernels.inc.h).
template <int NOBS, int NSLOT, typename PROG>
__global__ __launch_bounds__(1024) void fill_ordered_step_kernel(const SxSignalDesc* __restrict__ descs,
                                                                 const SxSegment* __restrict__ segs,
                                                                 const unsigned* __restrict__ blk_off, unsigned layout,
                                                                 unsigned dbg, unsigned nfill, SxTailArgs tail) {
  fill_step_body(nfill, tail, dbg, [&] {
    SxChainDescs one;
    one.d[0] = one.d[1] = one.d[2] = one.d[3] = descs;
    fill_ordered_body<NOBS, NSLOT, PROG, 1, true>(one, segs, blk_off, layout, dbg);
  });
}

template <int NOBS, int NSLOT, typename PROG, int PREW>
__global__ __launch_bounds__(1024) void fill_step_kernel(const SxSignalDesc* __restrict__ descs,
                                                         const SxSegment* __restrict__ segs,
                                                         const unsigned* __restrict__ blk_off, unsigned hist_words,
                                                         unsigned dbg, unsigned nfill, SxTailArgs tail) {
  fill_step_body(nfill, tail, dbg, [&] { fill_body<NOBS, NSLOT, true, PROG, PREW>(descs, segs, blk_off, hist_words, dbg); });
}

#if SXMC_WG_STAMPS
extern "C" {
__device__ unsigned long long sx_wg_stamps[3 * 4096];   // (the definition; fill_kernels.inc.h declares it)
}
extern "C" int sxmc_debug_read_wg_stamps(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sx_wg_stamps), sizeof(unsigned long long) * (size_t)n);
}
#endif

// ------------------------------------------------------------------------------------ pre-binning
// Builds the pre-binned column of one evaluator: for every sample, sum_k idx_k * stride_k over the
// observables in `mask` with the fill kernel's arithmetic (pdfz.cpp:388-398), or all ones when one of
// them is outside its domain (NaN included) or the row is padding.  width = bytes per sample.
__global__ __launch_bounds__(256) void prebin_kernel(const SxSignalDesc* __restrict__ dp, unsigned mask, int width,
                                                     void* out) {
  const SxSignalDesc& d = *dp;
  const unsigned long long npad = d.nvec * SXMC_VEC;
  const unsigned sentinel = width == 1 ? 0xFFu : width == 2 ? 0xFFFFu : 0xFFFFFFFFu;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += step) {
    unsigned val = sentinel;
    if (i < d.nsamples) {
      bool ok = true;
      int part = 0;
      for (int k = 0; k < d.nobs; k++) {
        if (!((mask >> k) & 1u)) continue;
        const double x = (double)to_global(d.cols)[(unsigned long long)k * d.col_pitch + i];
        ok = ok && (x >= d.lower[k]) && (x < d.upper[k]);
        part += (int)((x - d.lower[k]) * d.scale[k]) * d.bin_stride[k];
      }
      if (ok) val = (unsigned)part;
    }
    if (width == 1) static_cast<unsigned char*>(out)[i] = (unsigned char)val;
    else if (width == 2) static_cast<unsigned short*>(out)[i] = (unsigned short)val;
    else static_cast<unsigned*>(out)[i] = val;
  }
}

#if SXMC_MEASURE
// (measurement build only) test hook: out[k] = x[k]^i as the polynomial systematics form it
__global__ void pow_int_kernel(const double* __restrict__ x, int n, int i, double* __restrict__ out) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    double h = 1.0, l = 0.0;
    for (int t = 0; t < i; t++) pow_step(h, l, x[k]);
    out[k] = h;
  }
}
#endif

// ------------------------------------------------------------------------------------ layout
// Row-major [n][F] -> column-major with pitch; pads [n, nvec*4) with NaN in every column.
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ aos, float* __restrict__ cols,
                                                        unsigned long long n, int F,
                                                        unsigned long long pitch) {
  const unsigned long long npad = (n + SXMC_VEC - 1) / SXMC_VEC * SXMC_VEC;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += step) {
    for (int k = 0; k < F; k++) {
      cols[(unsigned long long)k * pitch + i] = (i < n) ? aos[i * F + k] : __int_as_float(0x7fc00000);
    }
  }
}

// GetSamples (pdfz.h:542-556): rows of nobs observables + the dataset id.
__global__ __launch_bounds__(256) void untranspose_obs_kernel(const float* __restrict__ cols, float* __restrict__ out,
                                                              unsigned long long n, int nobs,
                                                              unsigned long long pitch, float dataset) {
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    for (int k = 0; k < nobs; k++) out[i * (nobs + 1) + k] = cols[(unsigned long long)k * pitch + i];
    out[i * (nobs + 1) + nobs] = dataset;
  }
}

// A fill launch.  Raises the kernel's dynamic-LDS limit where the launch needs more than the default 48 KiB (on every
// such launch: the attribute is per device).  `fused`: the whole step in this launch -- the step end's workgroups
// (finisher + workers) are appended to the grid.  Otherwise, with the launch shape's two profiling events set, through
// hipExtLaunchKernelGGL, which stamps them with the dispatch's own begin and end (rocprofv3 --kernel-trace's duration).
template <typename K, typename... A>
hipError_t launch_fill(const SxLaunchShape& sh, K k, size_t lds, bool fused, hipStream_t s, A... args) {
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 grid(fused ? sh.grid + sh.tail_blocks : sh.grid), block(sh.threads);
  if (!fused && sh.ev_start && sh.ev_stop) {
    hipExtLaunchKernelGGL(k, grid, block, (std::uint32_t)lds, s, (hipEvent_t)sh.ev_start, (hipEvent_t)sh.ev_stop, 0u,
                          args...);
  } else {
    hipLaunchKernelGGL(k, grid, block, lds, s, args...);
  }
  return hipGetLastError();
}

using FillLauncher = hipError_t (*)(const SxLaunchShape&, const SxSignalDesc*, const SxSegment*, const unsigned*, hipStream_t);

// Rows, a pre-binned column, a bucketed table or rows with multiplicities (FORM = kPreWeighted): fill_kernel.  Fused with
// the step end there are the ordered programs (below) and, here, the LDS-histogram kernels of the EMPTY program over a
// pre-binned column (BASELINE config 2).
template <int NOBS, int NSLOT, bool LDS_HIST, typename PROG, int FORM = kFormRows>
hipError_t launch_fill_k(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                         const unsigned* blk_off, hipStream_t s) {
  const unsigned w = sx_fill_w(sh), dbg = (unsigned)sh.debug_mode;
  if constexpr (LDS_HIST && PROG::n == 0 && sx_form_prebinned(FORM)) {
    if (sh.tail) {
      return launch_fill(sh, fill_step_kernel<NOBS, NSLOT, PROG, FORM>, sh.lds_bytes, true, s, descs, segs, blk_off, w,
                         dbg, (unsigned)sh.grid, *static_cast<const SxTailArgs*>(sh.tail));
    }
  }
  if (sh.tail) return hipErrorInvalidValue;   // (the host asks sx_fill_has_step_form first)
  return launch_fill(sh, fill_kernel<NOBS, NSLOT, LDS_HIST, PROG, FORM>, sh.lds_bytes, false, s, descs, segs, blk_off, w,
                     dbg);
}

// The kernel that decodes the program at run time for this (nobs, nslot): over rows, or over rows with multiplicities.
template <int NOBS, int NSLOT>
FillLauncher decoded_launcher(bool lds_hist, bool weighted) {
  if (weighted) {
    return lds_hist ? launch_fill_k<NOBS, NSLOT, true, DynamicProg, kPreWeighted>
                    : launch_fill_k<NOBS, NSLOT, false, DynamicProg, kPreWeighted>;
  }
  return lds_hist ? launch_fill_k<NOBS, NSLOT, true, DynamicProg> : launch_fill_k<NOBS, NSLOT, false, DynamicProg>;
}

template <bool WEIGHTED>
hipError_t launch_fill_generic(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                               const unsigned* blk_off, hipStream_t s) {
  return sh.lds_hist ? launch_fill(sh, fill_kernel_generic<true, WEIGHTED>, sh.lds_bytes, false, s, descs, segs, blk_off,
                                   sx_fill_w(sh))
                     : launch_fill(sh, fill_kernel_generic<false, WEIGHTED>, (size_t)64, false, s, descs, segs, blk_off, 0u);
}

// entries per wave (keys + counts) of the per-wave LDS tables of the sparse counting over runs
unsigned sparse_smax(const SxLaunchShape& sh) { return (unsigned)(sh.sparse_lds_bytes / 4 / (sh.threads / 64u) / 2); }
template <int NOBS, int NSLOT, typename PROG>
hipError_t launch_fill_sparse_k(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                                const unsigned* blk_off, hipStream_t s) {
  return launch_fill(sh, fill_sparse_kernel<NOBS, NSLOT, PROG>, sh.sparse_lds_bytes, false, s, descs, segs, blk_off,
                     sparse_smax(sh), (unsigned)sh.debug_mode);
}

// a bucketed table with an ordered observable (fill_ordered_kernel, also fused with the step end) or a boxed one
template <int NOBS, int NSLOT, typename PROG, int FORM>
hipError_t launch_fill_ordered_k(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                                 const unsigned* blk_off, hipStream_t s) {
  const unsigned w = sx_fill_w(sh), dbg = (unsigned)sh.debug_mode;
  if constexpr (FORM == kFormBoxed) {
    return launch_fill(sh, fill_boxed_kernel<NOBS, NSLOT, PROG>, sh.lds_bytes, false, s, descs, segs, blk_off, w, dbg);
  } else if (sh.tail) {
    return launch_fill(sh, fill_ordered_step_kernel<NOBS, NSLOT, PROG>, sh.lds_bytes, true, s, descs, segs, blk_off, w, dbg,
                       (unsigned)sh.grid, *static_cast<const SxTailArgs*>(sh.tail));
  } else {
    return launch_fill(sh, fill_ordered_kernel<NOBS, NSLOT, PROG>, sh.lds_bytes, false, s, descs, segs, blk_off, w, dbg);
  }
}

// The programs built in.  A program is its words, one per systematic, over SLOTS: observables 0 .. nobs - 1 binned per
// sample, then the fields only read (ascending), then -- ordered and boxed entries -- that observable.  Anything else:
// hiprtc.  An entry of form kFormRows serves the table as it is, with a pre-binned column and bucketed, as far as it has
// the kernels (`HAS`); an ordered or boxed entry has the one kernel, histogram in LDS.
struct FillEntry {
  int form;                 // kFormRows, kFormOrdered or kFormBoxed
  int nobs, nslot, nops;
  unsigned ops[4];
  // [histogram in LDS / beyond it (dense global atomics or sparse event-bin counters) / bucketed table walked in runs, event
  // bins counted in per-wave LDS tables][form: rows, pre-binned 1 / 2 bytes per sample, bucketed, rows with multiplicities];
  // ordered and boxed: [0][0]
  FillLauncher fn[3][5];
};
static_assert(kFormRows == 0 && kFormPre1 == 1 && kFormPre2 == 2 && kFormBucketed == 3 && kPreWeighted == 4,
              "fn is indexed by these forms");
// kPre: LDS histogram, observables no systematic writes pre-binned; kBeyond: histogram beyond LDS, rows and pre-binned;
// kGran: bucketed table (every observable given is binned, + one offset per granule), histogram in LDS, beyond LDS, runs;
// kWeighted: rows with multiplicities, histogram in LDS and beyond it
enum : unsigned { kPre = 1, kBeyond = 2, kGran = 4, kWeighted = 8 };
template <int FORM, unsigned HAS, int NO, int NS, unsigned... OPS>
constexpr FillEntry fill_entry() {
  using P = StaticProg<OPS...>;
  FillEntry e = {FORM, NO, NS, (int)sizeof...(OPS), {OPS...}, {}};
  if constexpr (FORM != kFormRows) {
    e.fn[0][0] = launch_fill_ordered_k<NO, NS, P, FORM>;
  } else {
    e.fn[0][kFormRows] = launch_fill_k<NO, NS, true, P>;
    if constexpr (HAS & kPre) {
      e.fn[0][kFormPre1] = launch_fill_k<NO, NS, true, P, kFormPre1>;
      e.fn[0][kFormPre2] = launch_fill_k<NO, NS, true, P, kFormPre2>;
    }
    if constexpr (HAS & kBeyond) {
      e.fn[1][kFormRows] = launch_fill_k<NO, NS, false, P, kFormRows>;
      e.fn[1][kFormPre1] = launch_fill_k<NO, NS, false, P, kFormPre1>;
      e.fn[1][kFormPre2] = launch_fill_k<NO, NS, false, P, kFormPre2>;
    }
    if constexpr (HAS & kGran) {
      e.fn[0][kFormBucketed] = launch_fill_k<NO, NS, true, P, kFormBucketed>;
      e.fn[1][kFormBucketed] = launch_fill_k<NO, NS, false, P, kFormBucketed>;
      e.fn[2][kFormBucketed] = launch_fill_sparse_k<NO, NS, P>;
    }
    if constexpr (HAS & kWeighted) {
      e.fn[0][kPreWeighted] = launch_fill_k<NO, NS, true, P, kPreWeighted>;
      e.fn[1][kPreWeighted] = launch_fill_k<NO, NS, false, P, kPreWeighted>;
    }
  }
  return e;
}
#define SX_SHIFT(o) sx_op(SXMC_SYST_SHIFT, o)
#define SX_SCALE(o) sx_op(SXMC_SYST_SCALE, o)
#define SX_CTSC(o) sx_op(SXMC_SYST_CTSCALE, o)
#define SX_RES(o, e) sx_op(SXMC_SYST_RESOLUTION_SCALE, o, e)
#define SX_PROG(FORM, HAS, NO, NS, ...) fill_entry<FORM, HAS, NO, NS, ##__VA_ARGS__>()
const FillEntry kPrograms[] = {
    // no systematics at all (BASELINE config 2): EVERY observable is untouched, so the pre-binned column carries the
    // whole flat index and no float column is streamed at all -- 1 or 2 bytes per sample instead of 4 per observable
    SX_PROG(kFormRows, kPre, 1, 1), SX_PROG(kFormRows, kPre, 2, 2), SX_PROG(kFormRows, kPre, 3, 3),
    // 1-D (bench_sxmc pdfz: one shift; config/example.json: scale + resolution_scale).  These are also what a
    // bucketed higher-dimensional table with ONE observable written by systematics reduces to.
    SX_PROG(kFormRows, kGran, 1, 1, SX_SHIFT(0)), SX_PROG(kFormRows, kGran, 1, 1, SX_SCALE(0)),
    SX_PROG(kFormRows, kGran, 1, 1, SX_CTSC(0)), SX_PROG(kFormRows, kGran, 1, 1, SX_SHIFT(0), SX_SCALE(0)),
    SX_PROG(kFormRows, kGran, 1, 2, SX_RES(0, 1)), SX_PROG(kFormRows, kGran, 1, 2, SX_SCALE(0), SX_RES(0, 1)),
    SX_PROG(kFormRows, kGran, 1, 2, SX_SHIFT(0), SX_SCALE(0), SX_RES(0, 1)),
    // 2-D
    SX_PROG(kFormRows, kPre, 2, 2, SX_SHIFT(0)), SX_PROG(kFormRows, kPre, 2, 2, SX_SCALE(0)),
    SX_PROG(kFormRows, kPre, 2, 2, SX_SHIFT(1)), SX_PROG(kFormRows, kPre, 2, 3, SX_SCALE(0), SX_RES(0, 2)),
    // (also what BASELINE configs 3 and 5 reduce to once bucketed: e and r are written, the rest is not)
    SX_PROG(kFormRows, kGran, 2, 3, SX_SHIFT(1), SX_SCALE(0), SX_RES(0, 2)),
    // 3-D (BASELINE config 3: shift(r) + scale(e) + resolution_scale(e | e_true))
    SX_PROG(kFormRows, kPre, 3, 3, SX_SHIFT(0)), SX_PROG(kFormRows, kPre, 3, 3, SX_SCALE(0)),
    SX_PROG(kFormRows, kPre, 3, 4, SX_RES(0, 3)), SX_PROG(kFormRows, kPre, 3, 4, SX_SCALE(0), SX_RES(0, 3)),
    // (the one straight-line program of the WEIGHTED fill: decoded at run time it is bound by the scalar unit at this shape)
    SX_PROG(kFormRows, kPre | kBeyond | kWeighted, 3, 4, SX_SHIFT(1), SX_SCALE(0), SX_RES(0, 3)),
    // 5-D (BASELINE config 5: the same three systematics, histograms beyond LDS capacity)
    SX_PROG(kFormRows, kPre | kBeyond, 5, 6, SX_SHIFT(1), SX_SCALE(0), SX_RES(0, 5)),
    // ordered: one observable, one shift / scale (bench_sxmc pdfz): nothing is streamed but the granule words
    SX_PROG(kFormOrdered, 0, 0, 1, SX_SHIFT(0)), SX_PROG(kFormOrdered, 0, 0, 1, SX_SCALE(0)),
    // BASELINE configs 3 and 5 bucketed: e (scale + resolution_scale against e_true) binned per sample, r (shift) ordered
    SX_PROG(kFormOrdered, 0, 1, 3, SX_SHIFT(2), SX_SCALE(0), SX_RES(0, 1)),
    // boxed, BASELINE config 3 bucketed: r (shift) binned per sample, e (scale + resolution_scale against e_true) boxed
    SX_PROG(kFormBoxed, 0, 1, 3, SX_SHIFT(0), SX_SCALE(2), SX_RES(2, 1)),
};
constexpr int kNumPrograms = (int)(sizeof(kPrograms) / sizeof(kPrograms[0]));

// The launcher of built-in program `prog` for this form of table and histogram mode, or null.  `weighted`: the rows carry
// multiplicities (the rows form only).
FillLauncher program_launcher(int prog, int form, int lds_hist, int sparse_runs, bool weighted = false) {
  if (prog < 0 || prog >= kNumPrograms) return nullptr;
  const FillEntry& e = kPrograms[prog];
  const bool own = sx_form_ordered(form);   // (an entry of that form, its one kernel in [0][0])
  if (e.form != (own ? form : kFormRows) || form < kFormRows || (!own && form > kFormBucketed)) return nullptr;
  if (weighted && form != kFormRows) return nullptr;
  return e.fn[sparse_runs ? 2 : lds_hist ? 0 : 1][own ? 0 : weighted ? kPreWeighted : form];
}

}  // namespace

bool sx_fill_weighted_supports(int prog, int lds_hist) {
  return program_launcher(prog, kFormRows, lds_hist, 0, true) != nullptr;
}

bool sx_fill_has_specialization(int nobs, int nslot) {
  return nobs >= 1 && nobs <= 5 && nslot >= nobs && nslot <= nobs + 2;
}

int sx_fill_find_program(int form, int nobs, int nslot, int nops, const unsigned* ops) {
  const int entry_form = sx_form_ordered(form) ? form : kFormRows;
  for (int i = 0; i < kNumPrograms; i++) {
    const FillEntry& e = kPrograms[i];
    const bool shape = e.form == entry_form && e.nobs == nobs && e.nslot == nslot && e.nops == nops;
    if (shape && std::equal(ops, ops + nops, e.ops)) return i;
  }
  return -1;
}

bool sx_fill_supports(int prog, int form, int lds_hist, int sparse_runs) {
  return program_launcher(prog, form, lds_hist, sparse_runs) != nullptr;
}

// Does the launch described by `sh` also exist fused with the step end (see fill_step_kernel)?
bool sx_fill_has_step_form(const SxLaunchShape& sh) {
  if (sh.weighted) return false;   // (a weighted fill has no fused form: the step falls back to its separate step end)
  if (sh.rtc_fill || !sh.lds_hist || sh.grid <= 0 || !program_launcher(sh.static_prog, sh.form, 1, 0)) return false;
  return sh.form == kFormOrdered || (sx_form_prebinned(sh.form) && kPrograms[sh.static_prog].nops == 0);
}

hipError_t sx_launch_fill_sparse_runs(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                                      const unsigned* blk_off, hipStream_t s) {
  if (sh.grid <= 0) return hipSuccess;
  if (sh.rtc_sparse) {
    return sx_rtc_launch(sh.rtc_sparse, sh.grid, sh.threads, sh.sparse_lds_bytes, descs, segs, blk_off, sparse_smax(sh),
                         (unsigned)sh.debug_mode, s, sh.ev_start, sh.ev_stop);
  }
  const FillLauncher fn = program_launcher(sh.static_prog, sh.form, sh.lds_hist, 1);
  return fn ? fn(sh, descs, segs, blk_off, s) : hipErrorInvalidValue;
}

hipError_t sx_launch_prebin(const SxSignalDesc* d_desc, unsigned long long npad, unsigned mask, int width, void* out,
                            hipStream_t s) {
  if (npad == 0) return hipSuccess;
  unsigned long long bx = (npad + 255) / 256;
  if (bx > 8192) bx = 8192;
  hipLaunchKernelGGL(prebin_kernel, dim3((unsigned)bx), dim3(256), 0, s, d_desc, mask, width, out);
  return hipGetLastError();
}

// The fill of one launch class: the kernel specialised at run time, else the built-in program's for the table's form,
// else the kernel that decodes the program for this (nobs, nslot), else the generic one.
hipError_t sx_launch_fill(const SxLaunchShape& sh, const SxSignalDesc* descs, const SxSegment* segs,
                          const unsigned* blk_off, hipStream_t s) {
  if (sh.grid <= 0) return hipSuccess;
  // rows with multiplicities: the rows form only, never specialised at run time, never fused with the step end (the host
  // asks sx_fill_has_step_form first); its built-in program is the one the planner asked sx_fill_weighted_supports about
  if (sh.weighted && (sh.form != kFormRows || sh.rtc_fill || sh.tail)) return hipErrorInvalidValue;
  if (sh.rtc_fill) {
    return sx_rtc_launch(sh.rtc_fill, sh.grid, sh.threads, sh.lds_bytes, descs, segs, blk_off, sx_fill_w(sh),
                         (unsigned)sh.debug_mode, s, sh.ev_start, sh.ev_stop);
  }
  if (sx_form_ordered(sh.form) || (sh.static_prog >= 0 && (sh.weighted || sh.static_prog < kNumPrograms))) {
    const FillLauncher fn = program_launcher(sh.static_prog, sh.form, sh.lds_hist, 0, sh.weighted);
    return fn ? fn(sh, descs, segs, blk_off, s) : hipErrorInvalidValue;
  }
#define SX_CASE(NO, NS) \
  if (sh.nobs == NO && sh.nslot == NS) return decoded_launcher<NO, NS>(sh.lds_hist, sh.weighted)(sh, descs, segs, blk_off, s);
  SX_CASE(1, 1) SX_CASE(1, 2) SX_CASE(1, 3)
  SX_CASE(2, 2) SX_CASE(2, 3) SX_CASE(2, 4)
  SX_CASE(3, 3) SX_CASE(3, 4) SX_CASE(3, 5)
  SX_CASE(4, 4) SX_CASE(4, 5) SX_CASE(4, 6)
  SX_CASE(5, 5) SX_CASE(5, 6) SX_CASE(5, 7)
#undef SX_CASE
  return sh.weighted ? launch_fill_generic<true>(sh, descs, segs, blk_off, s)
                     : launch_fill_generic<false>(sh, descs, segs, blk_off, s);
}

hipError_t sx_launch_zero(const SxSignalDesc* d_descs, int nsig, int max_bins, unsigned* ticket, hipStream_t s) {
  if (nsig == 0) return hipSuccess;
  const int bx = sxstep::zero_blocks(max_bins, 256, 2048);
  hipLaunchKernelGGL(zero_kernel, dim3(bx, nsig), dim3(256), 0, s, d_descs, ticket);
  return hipGetLastError();
}

hipError_t sx_launch_eval_pdf(const SxSignalDesc* d_descs, int nsig, unsigned long long max_points,
                              hipStream_t s) {
  if (nsig == 0 || max_points == 0) return hipSuccess;
  unsigned long long bx = (max_points + 255) / 256;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(eval_pdf_kernel, dim3((unsigned)bx, nsig), dim3(256), 0, s, d_descs);
  return hipGetLastError();
}

#if SXMC_MEASURE
hipError_t sx_launch_pow_int(const double* x, int n, int i, double* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pow_int_kernel, dim3((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256), dim3(256), 0, s, x, n, i, out);
  return hipGetLastError();
}
#endif

hipError_t sx_launch_transpose(const float* aos, float* cols, unsigned long long nsamples, int nfields,
                               unsigned long long col_pitch, hipStream_t s) {
  unsigned long long npad = (nsamples + SXMC_VEC - 1) / SXMC_VEC * SXMC_VEC;
  if (npad == 0) return hipSuccess;
  unsigned long long bx = (npad + 255) / 256;
  if (bx > 8192) bx = 8192;
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)bx), dim3(256), 0, s, aos, cols, nsamples, nfields,
                     col_pitch);
  return hipGetLastError();
}

hipError_t sx_launch_untranspose_obs(const float* cols, float* out, unsigned long long nsamples, int nobs,
                                     unsigned long long col_pitch, float dataset, hipStream_t s) {
  if (nsamples == 0) return hipSuccess;
  unsigned long long bx = (nsamples + 255) / 256;
  if (bx > 8192) bx = 8192;
  hipLaunchKernelGGL(untranspose_obs_kernel, dim3((unsigned)bx), dim3(256), 0, s, cols, out, nsamples, nobs,
                     col_pitch, dataset);
  return hipGetLastError();
}
