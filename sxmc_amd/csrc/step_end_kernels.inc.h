// step_end_kernels.inc.h -- the end of a Metropolis step on gfx950, in every form: lookup + event sum over the rows,
// finish_nll_jump_pick_combo, and the clearing of histograms and normalisations the next evaluation would start with.
// Part of pdfz_kernels.hip's translation unit (included there behind fill_kernels.inc.h: the fused step's kernels are
// fills that call fill_step_body, and the measurement build's sx_wg_stamps array is written from both sides).
// The forms -- sequential in two launches (eval_nll_kernel, finish_zero_kernel), the ticket form (eval_nll_finish_kernel),
// one workgroup (tail_step_kernel), cooperative (step_end_kernel), fused with the fill (fill_step_body), the look-ahead
// pass in two launches (eval_nll2_kernel, finish2_zero_kernel) and cooperative (step_end2_kernel), the lockstep sets'
// (*_chains_kernel) -- walk the same chain bit for bit, and are put together from the same pieces, each written once:
//   eval_nll_block_part   a workgroup's block of the event sum
//   finish_step[_w]       finish_nll_jump_pick_combo over an SxStepArgs
//   clear_piece           a workgroup's share of one histogram's clearing
//   slot_publish, slot_await_empty, slots_collect   the cooperative forms' hand-over of the partial sums
//   lookahead_decide      the look-ahead pass's one or two steps
// The host's figures (grids, LDS, the words of the ticket block) are step_end_plan.h's.
#pragma once

#include <cstring>
#include <type_traits>
#include <vector>

#include "step_end_plan.h"

namespace {

using namespace sxfill;

// eval_pdf for all members fused with nll_event_chunks (nll_kernels.cpp:89-116): per event the
// lookup-table values are produced, stored (the lut is the API contract) and consumed in
// registers.  One partial sum per workgroup.  The kernel is a chain of dependent gathers
// (read_bins -> bins), so the per-member pointers are staged in LDS and the members are walked
// eight at a time with their loads issued together.
struct EvalMember {
  const int* read_bins;
  const unsigned* bins;
  float* out;
  long stride;
  double bin_norm;
  double coef;  // pars[sid] * nexpected * eff, the event-independent factor of nll_kernels.cpp:107
};
static_assert(sizeof(EvalMember) == sxstep::kEvalMemberBytes, "step_end_lds_bytes sizes the staging from this");

// Body shared by eval_nll_kernel and eval_nll_finish_kernel: returns the workgroup's partial event sum
// (valid in thread 0).  A row is an event -- or, with `weight`, a class of events that fall into the same
// bin of every member (the descriptors then point at the class tables and carry no lookup-table output):
// its log term counts weight[row] times.
// `ready`: called by every thread, once, after the loads that do not depend on the evaluation (the rows' event-bin
// tables, the first row's weight: set by SetEvalPoints) have been ISSUED and before anything the fill writes is read
// (histograms, normalisations): the fused step kernel waits there for the fill's workgroups, with those loads in
// flight under the wait.
//
// WHERE THE LOOK-UP POINTERS COME FROM (`mem`).  MembersFromDescs: the descriptor array in device memory (every form but one).
// MembersFromTable: also the by-value table of the cooperative step end (SxStepEndTable, at most 16 members, a kernel
// argument: the pointers to the rows' bins and to the histograms sit in scalar registers from the start).  With it the
// first row's gathers bins[rb] are issued as soon as rb is there, BEFORE the LDS staging of the members' factors and its
// barrier, which they need nothing from: the staging's own two dependent loads (descriptor j, then its normalisation;
// source_id, then the parameter) run beside the look-ups' two instead of between them.
// The arithmetic is one text for both: same expressions, same order, same partial sums.
struct MembersFromDescs {
  static constexpr bool kTable = false;
  const SxSignalDesc* __restrict__ descs;
};
struct MembersFromTable {
  static constexpr bool kTable = true;
  const SxSignalDesc* __restrict__ descs;
  const SxStepEndTable& t;
};

//
// THE ROW WEIGHT'S TYPE (`W`, taken from the pointer): unsigned -- how many events a class holds (the walks' default; null:
// every row counts once) -- or double: real event weights (sxmc_group_set_event_weights), per class their sum W_k in
// ascending event order, or per event when the rows are the events.  The term is (double)weight[row] * log(s), rounded
// once, in both; the unsigned instantiations are the text they were, and 1.0 weights give their bytes.
template <int BD = 0, typename W, typename Members, typename Ready>   // (BD > 0: the workgroup's logical size, see block_sum in nll_device.h)
__device__ __forceinline__ double eval_nll_block_part(const Members& mem, int nsig,
                                                      unsigned long long npoints, const W* __restrict__ weight,
                                                      const double* __restrict__ pars,
                                                      const double* __restrict__ nexpected,
                                                      const unsigned* __restrict__ n_mc,
                                                      const short* __restrict__ source_id,
                                                      const unsigned* __restrict__ norms, double* sh,
                                                      unsigned block_index, unsigned nblocks, Ready&& ready) {
  constexpr bool kTable = Members::kTable;
  double* s_wave = sh;  // [16] wave sums, then nsig EvalMember records
  EvalMember* s_mem = reinterpret_cast<EvalMember*>(sh + 16);
  const unsigned bdim = BD > 0 ? (unsigned)BD : blockDim.x;

  // The events' bin indices of the first members are requested before anything else: their addresses
  // need only the descriptors (uniform, scalar loads), so the loads fly while the per-member factors
  // below are fetched and staged.
  constexpr int U = 16;
  static_assert(!kTable || U == SXMC_STEP_END_MEMBERS, "the table holds one pass of members");
  int rb[U];
  unsigned long long i = (unsigned long long)block_index * bdim + threadIdx.x;
  // (clamped indices, no branches: all U table addresses are fetched together, then all U loads issued)
  auto load_read_bins = [&](unsigned long long ev, int j0) {
    const unsigned long long evc = ev < npoints ? ev : npoints - 1;
    gptr<const int> table[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      if constexpr (kTable) table[u] = to_global(mem.t.read_bins[u]);   // (entries past nsig repeat the last member)
      else table[u] = to_global(mem.descs[min(j0 + u, nsig - 1)].read_bins);
    }
#pragma unroll
    for (int u = 0; u < U; u++) rb[u] = table[u][evc];
#pragma unroll
    for (int u = 0; u < U; u++) rb[u] = (j0 + u < nsig && ev < npoints) ? rb[u] : -2;
  };
  auto bins_of = [&](int j0, int u) {
    if constexpr (kTable) return to_global(mem.t.bins[u]);
    else return to_global(s_mem[j0 + u].bins);
  };
  if (npoints == 0 || nsig <= 0) {   // uniform: nothing to look up
    ready();
    return 0.0;
  }
  load_read_bins(i, 0);
  static_assert(std::is_same<W, unsigned>::value || std::is_same<W, double>::value, "a count or a real weight");
  W wfirst = weight ? to_global(weight)[i < npoints ? i : npoints - 1] : W(1);
  unsigned count[U];   // (table form: the first row's counts are gathered before the staging barrier)

  // member j's staged record from its loaded inputs (one text for both forms)
  auto stage = [&](int j, const SxSignalDesc& d, unsigned normv, double volume, unsigned nj, unsigned nmc, double par,
                   double nexp) {
    s_mem[j].read_bins = d.read_bins;
    s_mem[j].bins = d.bins;
    s_mem[j].out = d.pdf_out;
    s_mem[j].stride = d.pdf_stride;
    s_mem[j].bin_norm = (double)normv * volume;
    const float eff = (float)(1.0 * nj / nmc);                       // nll_kernels.cpp:105
    s_mem[j].coef = par * nexp * eff;                                // left-to-right, :107
  };
  if constexpr (kTable) {
    // Lane j stages member j (at most 16: one pass).  Every lane loads, at a clamped index, so that the loads are one
    // instruction stream in the order of what they depend on: first what needs nothing (issued right behind the rows'
    // bins), then -- once the rows' bins are there -- the gathers, and beside them the staging's second level.
    const int j = min((int)threadIdx.x, nsig - 1);
    const SxSignalDesc& d = mem.descs[j];
    const unsigned* normp = d.norm;
    const double volume = d.bin_volume;
    const short sid = source_id[j];
    const unsigned nmc = n_mc[j];
    const double nexp = nexpected[j];
    ready();
    const unsigned nj = norms[j];
    const unsigned normv = *to_global(normp);
    const double par = pars[sid];
    // (the gathers without branches -- a row outside a member reads bin 0 and drops it: with every load issued on every
    //  path the waits below count exactly, and none of them stands between the gathers and the staging's loads)
#pragma unroll
    for (int u = 0; u < U; u++) count[u] = bins_of(0, u)[rb[u] >= 0 ? rb[u] : 0];
#pragma unroll
    for (int u = 0; u < U; u++) count[u] = (rb[u] >= 0) ? count[u] : 0u;
    // (no `if (threadIdx.x < nsig)`: the lanes past the last member store its record once more, the same values to the
    //  same place -- behind a branch the compiler moves every load above into it, BEHIND the gathers and their waits)
    stage(j, d, normv, volume, nj, nmc, par, nexp);
  } else {
    ready();
    for (int j = threadIdx.x; j < nsig; j += (int)bdim) {
      const SxSignalDesc& d = mem.descs[j];
      stage(j, d, *to_global((const unsigned*)d.norm), d.bin_volume, norms[j], n_mc[j], pars[source_id[j]], nexpected[j]);
    }
  }
#if SXMC_WG_STAMPS
  if (kTable && BD == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // (measurement build: the gathers have landed)
    SX_WG_STAMP(1);
  }
#endif
  __syncthreads();

  double sum = 0.0;
  bool requested = true;
  const unsigned long long step = (unsigned long long)nblocks * bdim;
  for (; i < npoints; i += step) {
    double s = 0.0;
    // (the row's weight is asked for before the gathers, not after the logarithm: one memory round trip less on a
    //  path that is nothing but round trips)
    const W wrow = requested ? wfirst : (weight ? to_global(weight)[i] : W(1));
    for (int j0 = 0; j0 < nsig; j0 += U) {
      const bool gathered = kTable && requested;
      if (!requested) load_read_bins(i, j0);
      requested = false;
      if (!gathered) {
#pragma unroll
        for (int u = 0; u < U; u++) count[u] = (rb[u] >= 0) ? bins_of(j0, u)[rb[u]] : 0u;
      }
#if SXMC_WG_STAMPS
      if (!kTable && BD == 0 && i < bdim * nblocks) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (measurement build: the gathers have landed)
        SX_WG_STAMP(1);
      }
#endif
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (j0 + u < nsig) {
          // pdfz.cpp:423-434: -2 -> 0, other negatives -> NaN, else (float)(bins / (norm * volume))
          float v;
          if (rb[u] == -2) v = 0.0f;
          else if (rb[u] < 0) v = __int_as_float(0x7fc00000);
          else v = (float)((double)count[u] / s_mem[j0 + u].bin_norm);
          if (s_mem[j0 + u].out) to_global(s_mem[j0 + u].out)[s_mem[j0 + u].stride * (long)i] = v;
          s = s + s_mem[j0 + u].coef * (double)(!isnan(v) ? v : 0.0f);
        }
      }
    }
    if (s > 0) sum += weight ? (double)wrow * log(s) : log(s);
  }

#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, kWave);
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) s_wave[wave] = sum;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    for (int w = 0; w < (int)(bdim / kWave); w++) t += s_wave[w];
  }
  return t;
}

template <int BD = 0, typename W, typename Ready>
__device__ __forceinline__ double eval_nll_block_part(const SxSignalDesc* __restrict__ descs, int nsig,
                                                      unsigned long long npoints, const W* __restrict__ weight,
                                                      const double* __restrict__ pars,
                                                      const double* __restrict__ nexpected,
                                                      const unsigned* __restrict__ n_mc,
                                                      const short* __restrict__ source_id,
                                                      const unsigned* __restrict__ norms, double* sh,
                                                      unsigned block_index, unsigned nblocks, Ready&& ready) {
  return eval_nll_block_part<BD>(MembersFromDescs{descs}, nsig, npoints, weight, pars, nexpected, n_mc, source_id, norms,
                                 sh, block_index, nblocks, ready);
}

template <int BD = 0, typename W>
__device__ __forceinline__ double eval_nll_block_part(const SxSignalDesc* __restrict__ descs, int nsig,
                                                      unsigned long long npoints, const W* __restrict__ weight,
                                                      const double* __restrict__ pars,
                                                      const double* __restrict__ nexpected,
                                                      const unsigned* __restrict__ n_mc,
                                                      const short* __restrict__ source_id,
                                                      const unsigned* __restrict__ norms, double* sh,
                                                      unsigned block_index, unsigned nblocks) {
  return eval_nll_block_part<BD>(descs, nsig, npoints, weight, pars, nexpected, n_mc, source_id, norms, sh, block_index,
                                 nblocks, [] {});
}

template <typename W>
__device__ __forceinline__ double eval_nll_block(const SxSignalDesc* __restrict__ descs, int nsig,
                                                 unsigned long long npoints, const W* __restrict__ weight,
                                                 const double* __restrict__ pars,
                                                 const double* __restrict__ nexpected,
                                                 const unsigned* __restrict__ n_mc,
                                                 const short* __restrict__ source_id,
                                                 const unsigned* __restrict__ norms, double* sh) {
  return eval_nll_block_part(descs, nsig, npoints, weight, pars, nexpected, n_mc, source_id, norms, sh, blockIdx.x,
                             gridDim.x);
}

// ------------------------------------------------------------------------------------ the shared pieces
// "nothing to wait for", "no stamp".  ONE type: finish_step_device_w keeps its staging in __shared__ arrays of its own, one
// set per instantiation, so two calls in a kernel share them only if their `wait`s are of one type.
struct Nothing {
  __device__ __forceinline__ void operator()() const {}
};

// finish_nll_jump_pick_combo over the step's arguments as the kernels hold them: the one place that spells out the
// fields of SxStepArgs.  `norms`: the normalisations of the candidate the step is decided from (the look-ahead pass's
// second step: candidate B's).  BD, R, `wait`: see finish_step_device_w (nll_device.h).
template <int BD = 0, int R = (BD > 0 ? 8 : 32), typename Wait>
__device__ __forceinline__ bool finish_step_w(size_t npartial, const double* sums, const SxStepArgs& a,
                                              const unsigned* norms, Wait&& wait) {
  return sxdev::finish_step_device_w<BD, R>(npartial, sums, a.nsignals, a.nsources, a.means, a.sigmas, a.rng,
                                            a.nll_current, a.nll_proposed, a.v_current, a.v_proposed, a.accepted,
                                            a.counter, a.jump_buffer, a.nparameters, a.jump_width, a.nexpected, a.n_mc,
                                            a.source_id, norms, a.factor, a.whitening, a.debug_mode != 0, wait);
}
template <int R = 32>
__device__ __forceinline__ bool finish_step(size_t npartial, const double* sums, const SxStepArgs& a,
                                            const unsigned* norms) {
  return finish_step_w<0, R>(npartial, sums, a, norms, Nothing{});
}
template <int R = 32>
__device__ __forceinline__ bool finish_step(size_t npartial, const double* sums, const SxStepArgs& a) {
  return finish_step<R>(npartial, sums, a, a.norms);
}

// Chunk `chunk` of `nchunks` of the clearing of one histogram (bins[0 .. n) <- 0) by a workgroup of bdim lanes: 16-byte
// stores, a lane's `nchunks * bdim` apart (hipMalloc'd: 256-byte aligned); chunk 0 also clears the n & 3 words behind
// the last whole store.
__device__ __forceinline__ void clear_piece(unsigned* bins, unsigned n, unsigned chunk, unsigned nchunks, unsigned bdim) {
  const unsigned n4 = n >> 2;
  uint4* b4 = reinterpret_cast<uint4*>(bins);
  const unsigned stride = nchunks * bdim;
  for (unsigned i = chunk * bdim + threadIdx.x; i < n4; i += stride) b4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (chunk == 0 && threadIdx.x < (n & 3u)) bins[(n4 << 2) + threadIdx.x] = 0u;
}

// THE HAND-OVER OF THE COOPERATIVE STEP ENDS (step_end_kernel, fill_step_body, step_end2_kernel; the protocol and why it
// has no fences and no counters: see step_end_kernel).  A slot holds a partial sum's bit pattern, or kSlotEmpty, or
// kSlotNaN for "my partial came out NaN" -- both markers are NaN patterns no stored partial can have.  Every wait is
// bounded: a lane that does not see its slot change within kEndSpinLimit polls (~0.3 s) counts a timeout and goes on.
constexpr unsigned kEndSpinLimit = 200000u;
constexpr unsigned long long kSlotEmpty = 0x7FF8DEADBEEF0001ull, kSlotNaN = 0x7FF8DEADBEEF0002ull;
// a worker (one lane) hands its partial over: ONE device-scope atomic store, the partial IS the message
__device__ __forceinline__ void slot_publish(unsigned long long* slot, double t) {
  __hip_atomic_store(slot, isnan(t) ? kSlotNaN : (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// ... and (the same lane) waits for the finisher to empty the slot: every partial is held, the look-ups are over, the
// histograms may be cleared.  false: gave up (counted in *timeouts).  `landed`: the measurement build's stamp.
template <typename Stamp = Nothing>
__device__ __forceinline__ bool slot_await_empty(unsigned long long* slot, unsigned* timeouts, Stamp landed = Stamp{}) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the store has landed before this lane starts reading the slot)
  landed();
  unsigned it = 0;
  for (; it < kEndSpinLimit; it++) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kSlotEmpty) break;
    __builtin_amdgcn_s_sleep(1);
  }
  if (it == kEndSpinLimit) __hip_atomic_fetch_add(timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return it < kEndSpinLimit;
}

// The finisher (every thread of the workgroup): lane i polls slot i of n until it holds a value, which goes to s_part[i]
// -- a slot never filled: 0, flagged in *timeouts, the step is not valid; kSlotNaN: the value of the last step whose
// partial was not NaN, which is what eval_nll_kernel's unwritten array element amounts to (nll_kernels.cpp:113-115 does
// not store a NaN partial).  Behind a barrier the slots are emptied -- for the next launch, and as the workers' signal.
// `held`: the measurement build's stamp.
template <typename Stamp = Nothing>
__device__ __forceinline__ void slots_collect(unsigned long long* slots, unsigned n, double* last_good, double* s_part,
                                              unsigned* timeouts, Stamp held = Stamp{}) {
  const unsigned i = threadIdx.x;
  if (i < n) {
    unsigned long long v = kSlotEmpty;
    for (unsigned it = 0; it < kEndSpinLimit; it++) {
      v = __hip_atomic_load(slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v != kSlotEmpty) break;
      __builtin_amdgcn_s_sleep(1);
    }
    double t;
    if (v == kSlotEmpty) {   // gave up
      __hip_atomic_fetch_add(timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      t = 0.0;
    } else if (v == kSlotNaN) {
      t = last_good[i];
    } else {
      t = __longlong_as_double((long long)v);
      last_good[i] = t;
    }
    s_part[i] = t;
  }
  __syncthreads();
  held();
  if (i < n) __hip_atomic_store(slots + i, kSlotEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// THE LOOK-AHEAD PASS'S DECISION (one workgroup; finish2_zero_kernel's workgroup 0, step_end2_kernel's finisher):
// finish_nll_jump_pick_combo for the step (candidate A = a.v_proposed) and, if that rejected and the walk may go on (the
// step count stays below *cap), for the next step: its proposal -- written into a.v_proposed by the first call -- IS
// the look-ahead vector (same current vector, same deviates, same arithmetic), so the second call runs on the same
// buffers with B's event sums and normalisations.  Then the next look-ahead vector is written to v_b and both groups'
// normalisations are cleared.  `wait`: as finish_step_w's; a pass launched after the walk reached its stop decides
// nothing but still calls it (the cooperative form's workers hand over and wait for their signal).
template <typename Wait>
__device__ __forceinline__ void lookahead_decide(size_t npartial, const double* sums_a, const double* sums_b,
                                                 const unsigned* norms_b, double* v_b, const int* cap,
                                                 const SxStepArgs& a, const SxSignalDesc* __restrict__ hist_a,
                                                 const SxSignalDesc* __restrict__ hist_b, int nsig, Wait&& wait) {
  __shared__ int s_before;
  if (threadIdx.x == 0) s_before = a.counter[0];
  __syncthreads();
  const int limit = cap ? cap[0] : 0x7FFFFFFF;
  if (s_before < limit) {
    const bool accepted = finish_step_w(npartial, sums_a, a, a.norms, wait);
    __syncthreads();
    if (!accepted && s_before + 1 < limit) {
      finish_step(npartial, sums_b, a, norms_b);
      __syncthreads();
    }
    sxdev::peek_next_proposal_device(a.nparameters, a.rng, a.jump_width, a.v_current, v_b);
  } else {
    wait();
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nsig; j += blockDim.x) {
    *hist_a[j].norm = 0u;
    *hist_b[j].norm = 0u;
  }
}

// ------------------------------------------------------------------------------------ sequential, ticket, look-ahead
template <typename W>
__global__ __launch_bounds__(256) void eval_nll_kernel(const SxSignalDesc* __restrict__ descs, int nsig,
                                                       unsigned long long npoints,
                                                       const W* __restrict__ weight,
                                                       const double* __restrict__ pars,
                                                       const double* __restrict__ nexpected,
                                                       const unsigned* __restrict__ n_mc,
                                                       const short* __restrict__ source_id,
                                                       const unsigned* __restrict__ norms,
                                                       double* __restrict__ sums) {
  extern __shared__ double sh[];
  const double t = eval_nll_block(descs, nsig, npoints, weight, pars, nexpected, n_mc, source_id, norms, sh);
  if (threadIdx.x == 0 && !isnan(t)) sums[blockIdx.x] = t;
}

// The whole end of an MCMC step in one launch: lookup + event partial sums as above, and the
// workgroup that arrives LAST (a ticket counter, no waiting, so no co-residency assumption) also runs
// finish_nll_jump_pick_combo.  Hand-off of the partial sums follows the agent-scope release/acquire
// recipe for gfx950: partial stored, drained and released by lane 0 before its ticket; the last arriver
// acquires (invalidating its CU's L1) before any of its lanes read the partials.
template <typename W>
__global__ __launch_bounds__(256) void eval_nll_finish_kernel(const SxSignalDesc* __restrict__ descs, int nsig,
                                                              unsigned long long npoints,
                                                              const W* __restrict__ weight, double* sums,
                                                              unsigned* ticket, SxStepArgs a) {
  extern __shared__ double sh[];
  const double t =
      eval_nll_block(descs, nsig, npoints, weight, a.v_proposed, a.nexpected, a.n_mc, a.source_id, a.norms, sh);
  int* s_last = reinterpret_cast<int*>(sh + 15);  // last wave-sum slot: at most 4 waves are in use
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = isnan(t) ? 0.0 : t;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = arrived == gridDim.x - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_last = last;
  }
  __syncthreads();
  if (!*s_last) return;
  __syncthreads();
  finish_step(gridDim.x, sums, a);
}

// LOOK-AHEAD WALK (sxmc_multigroup_lookahead_step_async).  A Metropolis step that rejects leaves the chain where it
// was, and the NEXT proposal -- current vector + jump width x the next deviates -- is then known before the
// step is decided.  One pass over the tables (the lockstep fill of two chains) evaluates the likelihood at BOTH
// the step's proposal A and that look-ahead vector B; the step end below decides the step from A and, if it
// rejected, the following step from B at once: 1 + P(reject) steps per pass, the chain -- every row of the
// jump buffer, every generator state -- exactly the sequential one (pre-fetching, Brockwell 2006).
// Lookup + event sums of both candidates in one launch: the first half of the grid works on A, the second on B.
__global__ __launch_bounds__(256) void eval_nll2_kernel(const SxSignalDesc* __restrict__ descs_a,
                                                        const SxSignalDesc* __restrict__ descs_b, int nsig,
                                                        unsigned long long npoints,
                                                        const unsigned* __restrict__ weight_a,
                                                        const unsigned* __restrict__ weight_b,
                                                        const double* __restrict__ pars_a,
                                                        const double* __restrict__ pars_b,
                                                        const double* __restrict__ nexpected,
                                                        const unsigned* __restrict__ n_mc,
                                                        const short* __restrict__ source_id,
                                                        const unsigned* __restrict__ norms_a,
                                                        const unsigned* __restrict__ norms_b,
                                                        double* __restrict__ sums_a, double* __restrict__ sums_b,
                                                        unsigned half) {
  extern __shared__ double sh[];
  const bool second = blockIdx.x >= half;
  // (eval_nll_block strides by gridDim.x: give each half its own picture of the grid)
  const double t = eval_nll_block_part(second ? descs_b : descs_a, nsig, npoints, second ? weight_b : weight_a,
                                       second ? pars_b : pars_a, nexpected, n_mc, source_id,
                                       second ? norms_b : norms_a, sh, second ? blockIdx.x - half : blockIdx.x, half);
  if (threadIdx.x == 0 && !isnan(t)) (second ? sums_b : sums_a)[second ? blockIdx.x - half : blockIdx.x] = t;
}

// Step end of the look-ahead walk + the clearing for the next pass.  Workgroup 0: lookahead_decide.  The other
// workgroups clear both candidates' histograms.
__global__ __launch_bounds__(256) void finish2_zero_kernel(const SxSignalDesc* __restrict__ descs_a,
                                                           const SxSignalDesc* __restrict__ descs_b, int nsig,
                                                           unsigned zblocks, size_t npartial, const double* sums_a,
                                                           const double* sums_b, const unsigned* norms_b, double* v_b,
                                                           const int* cap, SxStepArgs a) {
  if (blockIdx.x == 0) {
    lookahead_decide(npartial, sums_a, sums_b, norms_b, v_b, cap, a, descs_a, descs_b, nsig, Nothing{});
    return;
  }
  const unsigned b = blockIdx.x - 1u;
  const unsigned which = b / (zblocks * (unsigned)nsig);
  const unsigned bb = b - which * zblocks * (unsigned)nsig;
  const SxSignalDesc& d = (which ? descs_b : descs_a)[bb / zblocks];
  clear_piece(d.bins, (unsigned)d.total_nbins, bb % zblocks, zblocks, blockDim.x);
}

// first look-ahead vector of a walk (the state as sxmc_launch_pick_new_vector left it)
__global__ void peek_next_proposal_kernel(int nparameters, const sxmc_rng_state* rng, const float* jump_width,
                                          const double* v_current, double* out) {
  sxdev::peek_next_proposal_device(nparameters, rng, jump_width, v_current, out);
}

// The whole end of an MCMC step in ONE workgroup: lookup + event sum over the rows (events, or classes of events
// with a weight each), finish_nll_jump_pick_combo, and the clearing of histograms and normalisations the next
// evaluation would start with.  With a few thousand rows (event classes at BASELINE configs 1-3) the end of a step
// is a chain of memory latencies, not work: as its own kernels (lookup + event sum over ~40 workgroups, then the
// step end beside the zeroing) it costs two launch ramps, two kernel boundaries and a round trip of the partial
// sums through memory; here it is one ramp, and the step's other inputs are in flight under the gathers.
// `Wait`: Nothing, or NothingWeighted, a type of the same meaning.  WHY TWO TYPES: finish_step_device_w keeps its staging
// in static __shared__ arrays, one set per instantiation (see `Nothing`), and an instantiation used by TWO kernels has
// its arrays laid out in the module's shared LDS block instead of the one kernel's own.  OBSERVED (hipcc of ROCm 7, -O3,
// gfx950, `make asm`): with both weight types finishing through finish_step_w<0, 8, Nothing> the COUNTS' kernel lost 27-30
// of its 4 648 instructions -- phase B's addends were read from LDS in another order and its loop unrolled otherwise --,
// with a `Wait` type of its own per kernel it is the parent's code instruction for instruction, as the issue that
// brought the weights asked (this kernel IS the step end of small fits).  WHEN IT CAN GO: once the staging is owned by
// the calling kernel (passed in, not static), or when a diff of `make asm` shows the unsigned kernel unchanged
// without it; nothing but speed depends on it -- the results are the same either way.
struct NothingWeighted {
  __device__ __forceinline__ void operator()() const {}
};
template <typename W, typename Wait>
__global__ __launch_bounds__(1024) void tail_step_kernel(const SxSignalDesc* __restrict__ descs, int nsig,
                                                         unsigned long long npoints,
                                                         const W* __restrict__ weight, SxStepArgs a) {
  using sxstep::kStepSumRows;
  extern __shared__ double sh[];
  __shared__ double s_total;
  const double t =
      eval_nll_block(descs, nsig, npoints, weight, a.v_proposed, a.nexpected, a.n_mc, a.source_id, a.norms, sh);
  if (threadIdx.x == 0) {
    // The sequential step sums the rows in blocks of 128 (eval_nll_kernel: two waves each) and its finisher adds the
    // blocks' partial sums (block_sum).  This form is taken for at most 256 rows -- waves 0 .. 3 here, two such blocks
    // --, and (w0 + w1) + (w2 + w3) is not ((w0 + w1) + w2) + w3 to the last bit: beyond one block the waves' sums (still
    // in sh[0 .. 3]) are added block by block, so that the NLL is the sequential step's whatever form ends the step.
    // (the host's rule, step_end_takes_tail: at most kTailMaxLookups rows, two blocks of kStepSumRows rows = two waves each)
    static_assert(kStepSumRows == 2 * kWave && sxstep::kTailMaxLookups <= 2 * kStepSumRows, "waves 0 .. 3: two blocks of two waves");
    double total = t;
    if (npoints > kStepSumRows && nsig > 0) total = ((0.0 + sh[0]) + sh[1]) + ((0.0 + sh[2]) + sh[3]);
    s_total = isnan(total) ? 0.0 : total;   // (nll_kernels.cpp:113-115: a NaN partial is not stored)
  }
  __syncthreads();
  // (a launch bound of 1024 lanes, 128 registers: few of phase B's addends in registers)
  finish_step_w<0, 8>(1, &s_total, a, a.norms, Wait{});
  // (the normalisations were last read before the barriers inside finish_step_device)
  for (int j = 0; j < nsig; j++) {
    const SxSignalDesc& d = descs[j];
    clear_piece(d.bins, (unsigned)d.total_nbins, 0u, 1u, blockDim.x);
    if (threadIdx.x == 0) *d.norm = 0u;
  }
}

// finish_nll_jump_pick_combo (workgroup 0) and, beside it in the same launch, what zero_kernel does for
// the NEXT evaluation (all other workgroups): a walk that does not look at histograms or normalisations
// between steps saves a launch per step.  Workgroup 0 clears the normalisations itself, after it has read
// them; the other workgroups touch only the histograms (counters), which nothing reads at this point.
__global__ __launch_bounds__(256) void finish_zero_kernel(const SxSignalDesc* __restrict__ descs, int nsig,
                                                          unsigned zblocks, size_t npartial, const double* sums,
                                                          unsigned* ticket, SxStepArgs a) {
  if (blockIdx.x == 0) {
    finish_step(npartial, sums, a);
    __syncthreads();
    for (int j = threadIdx.x; j < nsig; j += blockDim.x) *descs[j].norm = 0u;
    if (threadIdx.x == 0 && ticket) *ticket = 0u;
    return;
  }
  const unsigned b = blockIdx.x - 1u;
  const SxSignalDesc& d = descs[b / zblocks];
  clear_piece(d.bins, (unsigned)d.total_nbins, b % zblocks, zblocks, blockDim.x);
}

// ------------------------------------------------------------------------------------ cooperative
// THE STEP END IN ONE LAUNCH (cooperative).  eval_nll_kernel + finish_zero_kernel are two launches whose work is a chain
// of memory round trips: at BASELINE config 3 they take 9.5 + 6.6 us, 18-20 us of a 150 us step with their boundaries
// (profiles/r03_c3_kernel_stats.csv), and more than the fill itself at config 2.  Earlier one-launch forms lost what
// the boundary saved: the LAST workgroup to arrive ran the whole step end cold (round 2: 15.7 against 14.7 us); one
// workgroup doing everything is far too slow beyond a few hundred look-ups; and a first cooperative form of this
// round -- partials published with a release fence and an arrival COUNTER, the finisher acquiring -- cost 17.8 us
// against 16.2 (profiles/r04_step_end_ab_*): a fence is an L2 write-back, the counter another round trip, the acquire
// an L2 invalidate, and a kernel boundary inside a replayed graph is only 0-1.3 us.  This form has no fences and no
// counters.  The roles are fixed at launch:
//   * workgroups 0 .. W-1 (the workers: W = the virtual blocks of the event sum, at most 128) do the look-ups and the
//     event sum exactly as eval_nll_kernel's workgroups do -- the same blocks of 128 rows, the same partial sums, so
//     the NLL and with it the chain stay bit-identical -- and hand their partial over with ONE device-scope atomic
//     store into their own 64-bit slot (the partial IS the message: nothing else of the worker's needs to be visible);
//   * workgroup W (the finisher) meanwhile does everything of finish_nll_jump_pick_combo that does not need the sums
//     (phase A of finish_step_device: every input loaded, the expected-rate and constraint terms, the next proposal's
//     deviates); then lane i polls slot i until it holds a value (device-scope atomic loads), the values go to LDS,
//     and what is left after the last worker's partial lands is a barrier, the reduction and phases B and C;
//   * once the finisher holds ALL partials -- every look-up is done, nothing reads the histograms any more -- it
//     empties the slots again, which is also the workers' signal: each polls its own slot until it is empty, then
//     clears its share of the histograms for the next evaluation (what zero_kernel would do) while the finisher
//     finishes; the finisher clears the normalisations, which it and the workers read.
// Waiting inside a kernel needs the waited-for workgroups to be resident or to become resident: the grid is at most
// 129 workgroups of 128 lanes with a few KB of LDS (the host takes this form only then), which the device holds many
// times over beside any fill kernel; the workers wait only for the finisher and the finisher only for the workers,
// all of one launch; and every wait is BOUNDED -- a lane that does not see its slot change within ~0.3 s gives up,
// counts a timeout (the ticket block's kTimeouts word, read by sxmc_group_step_end_timeouts) and goes on, so the grid
// always drains.

// The fused step's kernel argument: what step_end_kernel takes as arguments of its own (by value: pointers that arrive
// as arguments are uniform and known to be global).  (step_end_role takes the fields one by one, not this struct:
// building one from step_end_kernel's arguments cost step_end_kernel<true> three instructions.)
struct SxTailArgs {
  const SxSignalDesc* lookup_descs;
  const SxSignalDesc* hist_descs;
  int nsig;
  unsigned nvb, zblocks;
  unsigned real_weights;        // 0: `weight` points at unsigned counts (or is null); 1: at doubles (the same 8 bytes)
  unsigned long long npoints;
  const void* weight;
  unsigned long long* slots;
  double* last_good;
  unsigned* sync;
  SxStepArgs a;
};

// The roles of the cooperative step end.  `role` < W: worker `role`; `role` == W: the finisher.  BD > 0: the logical
// workgroup size when the roles run inside a launch of larger workgroups (fill_step_kernel); lanes >= BD have left.
// `ready`: called by every thread of the workgroup, once, before anything the fill writes is read (see
// eval_nll_block_part): nothing for step_end_kernel, whose launch follows the fill's; the wait for the fill's workgroups
// in fill_step_kernel.
// `lookup`: where the workers' members come from (MembersFromDescs / MembersFromTable, see eval_nll_block_part).
template <int BD, typename Wt, typename Members, typename Ready>
__device__ __forceinline__ void step_end_role(unsigned role, unsigned W, const Members& lookup,
                                              const SxSignalDesc* __restrict__ hist_descs, int nsig,
                                              unsigned long long npoints, const Wt* __restrict__ weight,
                                              unsigned long long* slots, double* last_good, unsigned* sync,
                                              unsigned nvb, unsigned zblocks, const SxStepArgs& a, double* sh,
                                              Ready&& ready) {
  const unsigned bdim = BD > 0 ? (unsigned)BD : blockDim.x;
  unsigned* const timeouts = sync + sxstep::kTimeouts;
  if (role == W) {
    // ---- the finisher (its phase A reads the normalisations: after the fill)
    ready();
    __shared__ double s_part[sxstep::kCoopMaxWorkers];
    // (the normalisations' addresses are fetched now, beside phase A's loads: the clearing stores below then wait for
    //  nothing -- lane j's member j; a group of more members than lanes goes round again after the step)
    unsigned* const my_norm = nsig > 0 ? hist_descs[min((int)threadIdx.x, nsig - 1)].norm : nullptr;
    // (only the staged form has read the normalisations by the time it waits: vectors longer than kStage total the NLL
    //  from them BEHIND the wait, nll_total_device, and are cleared behind the step as before)
    const bool clear_in_wait = a.nparameters <= sxdev::kStage && a.nsignals <= (size_t)sxdev::kStage;
    finish_step_w<BD>(nvb, s_part, a, a.norms, [&] {
      slots_collect(slots, nvb, last_good, s_part, timeouts, [] {
        if (BD == 0) SX_WG_STAMP(1);   // (measurement build: the finisher holds all partials)
      });
      // ... and nothing reads the normalisations any more either (the workers did while staging, this workgroup in
      // phase A, before the barrier in slots_collect): cleared here, out of the way of phases B and C, not behind them
      if (clear_in_wait && (int)threadIdx.x < nsig) *my_norm = 0u;
    });
    __syncthreads();
#if SXMC_MEASURE
    // (measurement build, the gated step: the next proposal is written -- published with a release at agent scope -- and
    // the fill that waits for it beside this kernel may read it)
    if (a.gate && threadIdx.x == 0) {
      __threadfence();
      __hip_atomic_store(a.gate, a.gate_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
    if (!clear_in_wait && (int)threadIdx.x < nsig) *my_norm = 0u;
    for (int j = (int)(threadIdx.x + bdim); j < nsig; j += (int)bdim) *hist_descs[j].norm = 0u;
    if (threadIdx.x == 0) sync[sxstep::kTicket] = 0u;   // (the ticket of the other step-end forms: as finish_zero_kernel leaves it)
    if (BD == 0) SX_WG_STAMP(2);
    return;
  }
  // ---- a worker: its virtual block of the event sum, as eval_nll_kernel's workgroup does it
  const unsigned vb = role;
  const double part = eval_nll_block_part<BD>(lookup, nsig, npoints, weight, a.v_proposed, a.nexpected, a.n_mc,
                                              a.source_id, a.norms, sh, vb, nvb, ready);
  __shared__ int s_clear;
  if (threadIdx.x == 0) slot_publish(slots + vb, part);
  // What the clearing needs of the histograms' descriptors -- address and bin count per member -- is fetched BEFORE the
  // wait for the finisher's signal (behind the slot's store, which is on its way) and parked in LDS (over the staged member
  // records, which nothing reads any more: every lane is past the event sum's last barrier), so that the clearing stores
  // issue the moment the slot reads empty, not two scalar loads and a wait per piece later.
  struct HistRange {
    unsigned* bins;
    unsigned n, pad;
  };
  static_assert(sizeof(HistRange) <= sizeof(EvalMember), "parked over the member records");
  HistRange* const s_hist = reinterpret_cast<HistRange*>(sh + 16);
  for (int j = threadIdx.x; j < nsig; j += (int)bdim) {
    s_hist[j].bins = hist_descs[j].bins;
    s_hist[j].n = (unsigned)hist_descs[j].total_nbins;
  }
  if (threadIdx.x == 0) {
    s_clear = slot_await_empty(slots + vb, timeouts, [] {
      if (BD == 0) SX_WG_STAMP(2);   // (measurement build: the worker's slot is stored)
    }) ? 1 : 0;
  }
  __syncthreads();
  if (!s_clear) return;
  const unsigned npieces = zblocks * (unsigned)nsig;
  for (unsigned p = role; p < npieces; p += W) {
    const HistRange d = s_hist[p / zblocks];
    clear_piece(d.bins, d.n, p % zblocks, zblocks, bdim);
  }
}

// TABLE: the workers' look-up pointers arrive by value (`table`: groups of up to 16 members -- the flagship's and config
// 2's step end) beside `lookup_descs`; otherwise everything comes from `lookup_descs`, and `table` is not read.
template <bool TABLE, typename Wt = unsigned>
__global__ __launch_bounds__(128) void step_end_kernel(const SxSignalDesc* __restrict__ lookup_descs,
                                                       const SxSignalDesc* __restrict__ hist_descs, int nsig,
                                                       unsigned long long npoints, const Wt* __restrict__ weight,
                                                       unsigned long long* slots, double* last_good, unsigned* sync,
                                                       unsigned nvb, unsigned zblocks, SxStepArgs a, SxStepEndTable table) {
  extern __shared__ double sh[];
  SX_WG_STAMP(0);   // (measurement build: entry; worker: gathers landed / finisher: all partials held; slot stored / exit)
  if constexpr (TABLE) {
    step_end_role<0>(blockIdx.x, gridDim.x - 1u, MembersFromTable{lookup_descs, table}, hist_descs, nsig, npoints, weight, slots,
                     last_good, sync, nvb, zblocks, a, sh, [] {});
  } else {
    step_end_role<0>(blockIdx.x, gridDim.x - 1u, MembersFromDescs{lookup_descs}, hist_descs, nsig, npoints, weight, slots,
                     last_good, sync, nvb, zblocks, a, sh, [] {});
  }
}

// THE WHOLE STEP IN ONE LAUNCH: fill_step_kernel = a fill kernel + the roles above as extra workgroups of the SAME launch.
// What is left between the fill and the cooperative step end as two launches is the second kernel's ramp (~2.5 us), the
// gap before it (~1.3 us) and its first loads (descriptors, event-bin tables, weights, staged factors: two memory round
// trips) -- all of which can sit under the fill's tail, whose workgroups finish over ~8 us.  Blocks
// 0 .. nfill-1 are the fill's workgroups, unchanged, each counting itself done (after its flush has landed: every lane
// waits for its own atomics, then one device-scope increment); block nfill is the finisher, blocks nfill+1 .. the
// workers.  A role workgroup starts on a CU as soon as a fill workgroup has left it (they all carry the fill's LDS
// allotment, one workgroup per CU), does what does not depend on the histograms, waits for the count to reach nfill,
// acquires, and goes on as step_end_role.  Who waits for whom: the roles for fill workgroups and the workers for the
// finisher -- all EARLIER blocks of the same launch, which the dispatcher has started before them; the fill
// workgroups wait for nobody; only the finisher (one workgroup per launch) waits for later blocks.  So the launch
// makes progress whatever else shares the device, and every wait is bounded as in step_end_kernel.
// The roles run with the fill's workgroup size; lanes >= 128 leave at once and the rest behave as a workgroup of 128
// (BD = 128 throughout: the same virtual blocks, partial sums and reduction tree as step_end_kernel -- bit-identical).
template <typename Fill>
__device__ __forceinline__ void fill_step_body(unsigned nfill, const SxTailArgs& t, unsigned dbg, Fill&& fill) {
  unsigned* const done = t.sync + sxstep::kFillDone;
  if (blockIdx.x < nfill) {
    fill();
    // this workgroup's flush has landed before it counts itself done: every lane waits for the acknowledgement of its
    // own device-scope atomics (they are performed at the memory side: acknowledged = performed), then one lane adds
    // to the count at the same scope.  (No release fence: on gfx950 that is a write-back of the XCD's whole L2, which
    // every workgroup would pay at the tail of the launch, and nothing but those atomics has to be published.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (threadIdx.x >= 128u) return;   // (whole waves: the roles are workgroups of 128)
  if (sxfill::sx_dbg(dbg) & 8u) return;   // measurement build only (RESULTS ARE WRONG): the fill's part of the launch alone
  SX_WG_STAMP(0);                    // (measurement build: a role's entry, its sight of the fill's end, its exit)
  extern __shared__ double sh_tail[];
  const unsigned role_index = blockIdx.x - nfill;            // 0: the finisher, 1 ..: workers
  const unsigned W = t.nvb;
  const unsigned role = role_index == 0 ? W : role_index - 1u;
  // The wait for the fill.  No acquire fence after it: what the roles read of the fill's -- counters and normalisations,
  // all written by device-scope atomics at the memory side -- is read here for the first time since the launch began
  // (the launch itself started with the caches invalidated, and the fill's workgroups read none of it), so no stale
  // copy can sit in this CU's L1 or this XCD's L2; and an agent-scope acquire on gfx950 invalidates the XCD's WHOLE L2,
  // once per role workgroup, under the other roles' look-ups (measured: the roles took 28 us instead of 14).
  auto fill_done = [&] {
    if (threadIdx.x == 0) {
      unsigned it = 0;
      for (; it < kEndSpinLimit; it++) {
        if (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nfill) break;
        __builtin_amdgcn_s_sleep(1);
      }
      if (it == kEndSpinLimit) {
        __hip_atomic_fetch_add(t.sync + sxstep::kTimeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    SX_WG_STAMP(1);
    __syncthreads();
  };
  // (uniform, a kernel argument.  Real event weights: the WORKERS take the roles' double instantiation; the finisher never
  //  sees the weights and stays in the other, so that the kernel holds one set of the finisher's staging arrays in LDS)
  if (t.real_weights && role != W) {
    step_end_role<128>(role, W, MembersFromDescs{t.lookup_descs}, t.hist_descs, t.nsig, t.npoints,
                       static_cast<const double*>(t.weight), t.slots, t.last_good, t.sync, t.nvb, t.zblocks, t.a, sh_tail, fill_done);
  } else {
    step_end_role<128>(role, W, MembersFromDescs{t.lookup_descs}, t.hist_descs, t.nsig, t.npoints,
                       static_cast<const unsigned*>(t.weight), t.slots, t.last_good, t.sync, t.nvb, t.zblocks, t.a, sh_tail, fill_done);
  }
  // the finisher is the last to need the count of this launch: it zeroes it for the next one
  if (role == W && threadIdx.x == 0) __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  SX_WG_STAMP(2);
}

// The look-ahead pass's step end as ONE cooperative launch: eval_nll2_kernel + finish2_zero_kernel with the hand-over
// of step_end_kernel.  Workers 0 .. nvb-1 sum candidate A's virtual blocks, nvb .. 2 nvb-1 candidate B's (each exactly
// as eval_nll2_kernel's workgroups do: same blocks, same partial sums -- the walk stays the sequential chain bit for
// bit); slot w belongs to worker w.  The finisher (workgroup 2 nvb) does phase A of the step's
// finish_nll_jump_pick_combo while they work, then lane w polls slot w (2 nvb <= 128 lanes); once it holds every
// partial of BOTH candidates it empties the slots -- the workers' signal to clear both candidates' histograms -- and
// goes on as finish2_zero_kernel's workgroup 0 (lookahead_decide).
__global__ __launch_bounds__(128) void step_end2_kernel(const SxSignalDesc* __restrict__ lookup_a,
                                                        const SxSignalDesc* __restrict__ lookup_b,
                                                        const SxSignalDesc* __restrict__ hist_a,
                                                        const SxSignalDesc* __restrict__ hist_b, int nsig,
                                                        unsigned long long npoints, const unsigned* __restrict__ weight_a,
                                                        const unsigned* __restrict__ weight_b, unsigned long long* slots,
                                                        double* last_good, unsigned* sync, unsigned nvb, unsigned zblocks,
                                                        const unsigned* norms_b, double* v_b, const int* cap, SxStepArgs a) {
  extern __shared__ double sh[];
  const unsigned W = gridDim.x - 1u;   // == 2 * nvb
  unsigned* const timeouts = sync + sxstep::kTimeouts;
  if (blockIdx.x == W) {
    // ---- the finisher
    __shared__ double s_part[sxstep::kCoopMaxWorkers];   // [0, nvb): candidate A's partial sums, [nvb, 2 nvb): candidate B's
    lookahead_decide(nvb, s_part, s_part + nvb, norms_b, v_b, cap, a, hist_a, hist_b, nsig,
                     [&] { slots_collect(slots, W, last_good, s_part, timeouts); });
    return;
  }
  // ---- a worker
  const bool second = blockIdx.x >= nvb;
  const unsigned vb = second ? blockIdx.x - nvb : blockIdx.x;
  const double t = eval_nll_block_part(second ? lookup_b : lookup_a, nsig, npoints, second ? weight_b : weight_a,
                                       second ? v_b : a.v_proposed, a.nexpected, a.n_mc, a.source_id,
                                       second ? norms_b : a.norms, sh, vb, nvb);
  __shared__ int s_clear;
  if (threadIdx.x == 0) {
    slot_publish(slots + blockIdx.x, t);
    s_clear = slot_await_empty(slots + blockIdx.x, timeouts) ? 1 : 0;
  }
  __syncthreads();
  if (!s_clear) return;
  const unsigned npieces = 2u * zblocks * (unsigned)nsig;
  for (unsigned p = blockIdx.x; p < npieces; p += W) {
    const unsigned which = p / (zblocks * (unsigned)nsig);
    const unsigned q = p - which * zblocks * (unsigned)nsig;
    const SxSignalDesc& d = (which ? hist_b : hist_a)[q / zblocks];
    clear_piece(d.bins, (unsigned)d.total_nbins, q % zblocks, zblocks, blockDim.x);
  }
}

// ------------------------------------------------------------------------------------ lockstep sets
// LOCKSTEP SETS: the step ends of all chains of a set in two launches instead of two per chain.  The chains have
// their own events (event classes, weights), parameter vectors, generators and jump buffers, so nothing is shared
// but the launch: chain = blockIdx.y, and inside a chain every workgroup does exactly what it does in
// eval_nll_kernel / finish_zero_kernel launched for that chain alone (same blocks of the event sum, same order of
// the partial sums) -- the chains stay bit-identical to chains stepped one at a time.  These kernels are a few
// microseconds of memory latency each; C chains cost the latency once instead of C times.
__global__ __launch_bounds__(256) void eval_nll_chains_kernel(SxChainEnds e, int nsig) {
  extern __shared__ double sh[];
  const SxChainEnd& c = e.c[blockIdx.y];
  if (blockIdx.x >= c.nblocks) return;   // (uniform: a chain with fewer rows than the set's largest)
  const double t = eval_nll_block_part(c.lookup_descs, nsig, c.nrows, c.weight, c.a.v_proposed, c.a.nexpected, c.a.n_mc,
                                       c.a.source_id, c.a.norms, sh, blockIdx.x, c.nblocks);
  if (threadIdx.x == 0 && !isnan(t)) c.sums[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void finish_zero_chains_kernel(SxChainEnds e, int nsig, unsigned zblocks) {
  const SxChainEnd& c = e.c[blockIdx.y];
  if (blockIdx.x == 0) {
    finish_step(c.nblocks, c.sums, c.a);
    __syncthreads();
    for (int j = threadIdx.x; j < nsig; j += blockDim.x) *c.hist_descs[j].norm = 0u;
    if (threadIdx.x == 0 && c.ticket) *c.ticket = 0u;
    return;
  }
  const unsigned b = blockIdx.x - 1u;
  const SxSignalDesc& d = c.hist_descs[b / zblocks];
  clear_piece(d.bins, (unsigned)d.total_nbins, b % zblocks, zblocks, blockDim.x);
}

}  // namespace

// ------------------------------------------------------------------------------------ launchers
size_t sx_tail_args_bytes() { return sizeof(SxTailArgs); }
// Fills the host image of a group's SxTailArgs (the device struct is private to this file).
void sx_tail_args_fill(void* image, const SxSignalDesc* lookup_descs, const SxSignalDesc* hist_descs, int nsig,
                       int max_bins, unsigned long long npoints, const unsigned* weight, const double* real_weight,
                       unsigned long long* slots, double* last_good, unsigned* sync, int nvb, const SxStepArgs& a) {
  SxTailArgs t;
  std::memset(&t, 0, sizeof t);   // (padding too: the host compares images bytewise to see whether to upload again)
  t.lookup_descs = lookup_descs;
  t.hist_descs = hist_descs;
  t.nsig = nsig;
  t.nvb = (unsigned)nvb;
  t.zblocks = (unsigned)sxstep::zero_blocks(max_bins, 128);   // (the roles are workgroups of 128)
  t.npoints = npoints;
  t.weight = real_weight ? static_cast<const void*>(real_weight) : static_cast<const void*>(weight);
  t.real_weights = real_weight ? 1u : 0u;
  t.slots = slots;
  t.last_good = last_good;
  t.sync = sync;
  std::memcpy(&t.a, &a, sizeof a);
  std::memcpy(image, &t, sizeof t);
}

// (each launcher of a row sum twice, by the weight's type: counts or real weights -- one text)
template <typename W>
hipError_t sx_launch_eval_nll(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                              const W* weight, const double* pars, const double* nexpected, const unsigned* n_mc,
                              const short* source_id, const unsigned* norms, double* sums,
                              int grid, int block, hipStream_t s) {
  hipLaunchKernelGGL(eval_nll_kernel<W>, dim3(grid), dim3(block), sxstep::step_end_lds_bytes(nsig), s, d_descs, nsig, npoints,
                     weight, pars, nexpected, n_mc, source_id, norms, sums);
  return hipGetLastError();
}

template <typename W>
hipError_t sx_launch_eval_nll_finish(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                                      const W* weight, double* sums, unsigned* ticket, const SxStepArgs& a,
                                      int grid, int block, hipStream_t s) {
  hipLaunchKernelGGL(eval_nll_finish_kernel<W>, dim3(grid), dim3(block), sxstep::step_end_lds_bytes(nsig), s, d_descs, nsig,
                     npoints, weight, sums, ticket, a);
  return hipGetLastError();
}

hipError_t sx_launch_eval_nll2(const SxSignalDesc* descs_a, const SxSignalDesc* descs_b, int nsig,
                               unsigned long long npoints, const unsigned* weight_a, const unsigned* weight_b,
                               const double* pars_a, const double* pars_b, const double* nexpected,
                               const unsigned* n_mc, const short* source_id, const unsigned* norms_a,
                               const unsigned* norms_b, double* sums_a, double* sums_b, int half, int block,
                               hipStream_t s) {
  hipLaunchKernelGGL(eval_nll2_kernel, dim3(2 * half), dim3(block), sxstep::step_end_lds_bytes(nsig), s, descs_a, descs_b,
                     nsig, npoints, weight_a, weight_b, pars_a, pars_b, nexpected, n_mc, source_id, norms_a, norms_b,
                     sums_a, sums_b, (unsigned)half);
  return hipGetLastError();
}

hipError_t sx_launch_finish2_zero(const SxSignalDesc* descs_a, const SxSignalDesc* descs_b, int nsig, int max_bins,
                                  size_t npartial, const double* sums_a, const double* sums_b, const unsigned* norms_b,
                                  double* v_b, const int* cap, const SxStepArgs& a, int block, hipStream_t s) {
  const unsigned zb = (unsigned)sxstep::zero_blocks(max_bins, block);
  hipLaunchKernelGGL(finish2_zero_kernel, dim3(1 + 2u * zb * (unsigned)nsig), dim3(block), 0, s, descs_a, descs_b, nsig,
                     zb, npartial, sums_a, sums_b, norms_b, v_b, cap, a);
  return hipGetLastError();
}

hipError_t sx_launch_peek_next_proposal(int nparameters, const sxmc_rng_state* rng, const float* jump_width,
                                        const double* v_current, double* out, hipStream_t s) {
  hipLaunchKernelGGL(peek_next_proposal_kernel, dim3(1), dim3(256), 0, s, nparameters, rng, jump_width, v_current, out);
  return hipGetLastError();
}

template <typename W>
hipError_t sx_launch_tail_step(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                               const W* weight, const SxStepArgs& a, hipStream_t s) {
  using Wait = typename std::conditional<std::is_same<W, double>::value, NothingWeighted, Nothing>::type;
  hipLaunchKernelGGL((tail_step_kernel<W, Wait>), dim3(1), dim3(1024), sxstep::step_end_lds_bytes(nsig), s, d_descs, nsig,
                     npoints, weight, a);
  return hipGetLastError();
}

hipError_t sx_launch_finish_zero(const SxSignalDesc* d_descs, int nsig, int max_bins, size_t npartial,
                                 const double* sums, unsigned* ticket, const SxStepArgs& a, int block, hipStream_t s) {
  const unsigned zb = (unsigned)sxstep::zero_blocks(max_bins, block);
  hipLaunchKernelGGL(finish_zero_kernel, dim3(1 + zb * (unsigned)nsig), dim3(block), 0, s, d_descs, nsig, zb, npartial,
                     sums, ticket, a);
  return hipGetLastError();
}

template <typename W>
hipError_t sx_launch_step_end(const SxSignalDesc* lookup_descs, const SxSignalDesc* hist_descs, int nsig, int max_bins,
                              unsigned long long npoints, const W* weight, unsigned long long* slots,
                              double* last_good, unsigned* sync, int nvb, const SxStepArgs& a, hipStream_t s,
                              const SxStepEndTable* table) {
  const int block = 128;   // (the rows of a virtual block of the event sum: eval_nll_kernel's workgroup)
  const size_t shmem = sxstep::step_end_lds_bytes(nsig);
  const unsigned zb = (unsigned)sxstep::zero_blocks(max_bins, block);
  if (table && nsig <= SXMC_STEP_END_MEMBERS) {
    hipLaunchKernelGGL((step_end_kernel<true, W>), dim3((unsigned)nvb + 1u), dim3(block), shmem, s, lookup_descs, hist_descs,
                       nsig, npoints, weight, slots, last_good, sync, (unsigned)nvb, zb, a, *table);
  } else {
    hipLaunchKernelGGL((step_end_kernel<false, W>), dim3((unsigned)nvb + 1u), dim3(block), shmem, s, lookup_descs, hist_descs,
                       nsig, npoints, weight, slots, last_good, sync, (unsigned)nvb, zb, a, SxStepEndTable{});
  }
  return hipGetLastError();
}

hipError_t sx_launch_step_end2(const SxSignalDesc* lookup_a, const SxSignalDesc* lookup_b, const SxSignalDesc* hist_a,
                               const SxSignalDesc* hist_b, int nsig, int max_bins, unsigned long long npoints,
                               const unsigned* weight_a, const unsigned* weight_b, unsigned long long* slots,
                               double* last_good, unsigned* sync, int nvb, const unsigned* norms_b, double* v_b,
                               const int* cap, const SxStepArgs& a, hipStream_t s) {
  const int block = 128;
  hipLaunchKernelGGL(step_end2_kernel, dim3(2u * (unsigned)nvb + 1u), dim3(block), sxstep::step_end_lds_bytes(nsig), s,
                     lookup_a, lookup_b, hist_a, hist_b, nsig, npoints, weight_a, weight_b, slots, last_good, sync,
                     (unsigned)nvb, (unsigned)sxstep::zero_blocks(max_bins, block), norms_b, v_b, cap, a);
  return hipGetLastError();
}

#define SX_ROW_SUM_LAUNCHERS(W)                                                                                            \
  template hipError_t sx_launch_eval_nll<W>(const SxSignalDesc*, int, unsigned long long, const W*, const double*,        \
                                            const double*, const unsigned*, const short*, const unsigned*, double*, int,  \
                                            int, hipStream_t);                                                            \
  template hipError_t sx_launch_eval_nll_finish<W>(const SxSignalDesc*, int, unsigned long long, const W*, double*,       \
                                                   unsigned*, const SxStepArgs&, int, int, hipStream_t);                  \
  template hipError_t sx_launch_tail_step<W>(const SxSignalDesc*, int, unsigned long long, const W*, const SxStepArgs&,   \
                                             hipStream_t);                                                                \
  template hipError_t sx_launch_step_end<W>(const SxSignalDesc*, const SxSignalDesc*, int, int, unsigned long long,       \
                                            const W*, unsigned long long*, double*, unsigned*, int, const SxStepArgs&,    \
                                            hipStream_t, const SxStepEndTable*);
SX_ROW_SUM_LAUNCHERS(unsigned)
SX_ROW_SUM_LAUNCHERS(double)
#undef SX_ROW_SUM_LAUNCHERS

// Workgroups of the cooperative step end the device holds at once (the runtime's occupancy figure for step_end_kernel
// with this launch's LDS x the CU count; 0: could not be asked) -- what the host's residency check counts against
int sx_step_end_resident_capacity(int nsig, int cus) {
  const size_t shmem = sxstep::step_end_lds_bytes(nsig);
  int per_cu = 0;
  const hipError_t e = nsig <= SXMC_STEP_END_MEMBERS
                           ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, step_end_kernel<true>, 128, shmem)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, step_end_kernel<false>, 128, shmem);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return per_cu * cus;
}

// the cooperative step end's slots start out empty
hipError_t sx_step_end_slots_init(unsigned long long* slots, double* last_good, int n) {
  std::vector<unsigned long long> h((size_t)n, kSlotEmpty);
  hipError_t e = hipMemcpy(slots, h.data(), sizeof(unsigned long long) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(last_good, 0, sizeof(double) * (size_t)n);
  return e;
}

hipError_t sx_launch_chain_ends(const SxChainEnds& e, int nchains, int nsig, int max_bins, int block, hipStream_t s) {
  unsigned widest = 1;
  for (int c = 0; c < nchains; c++) widest = e.c[c].nblocks > widest ? e.c[c].nblocks : widest;
  hipLaunchKernelGGL(eval_nll_chains_kernel, dim3(widest, (unsigned)nchains), dim3(block), sxstep::step_end_lds_bytes(nsig),
                     s, e, nsig);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  const unsigned zb = (unsigned)sxstep::zero_blocks(max_bins, block);
  hipLaunchKernelGGL(finish_zero_chains_kernel, dim3(1 + zb * (unsigned)nsig, (unsigned)nchains), dim3(block), 0, s, e,
                     nsig, zb);
  return hipGetLastError();
}
