// nll_device.h -- device functions of the NLL half of the MCMC step, shared by nll_kernels.hip (the
// reference's separate entry points) and step_end_kernels.inc.h (the fused lookup + event sum + step end).
// See nll_kernels.hip for the reference lines each one restates.
#pragma once

#include "sxmc_device.h"

#pragma clang fp contract(off)

namespace sxdev {

constexpr int kWave = 64;

// ------------------------------------------------------------------------------------ RNG
struct Philox4 {
  unsigned x, y, z, w;
};

__device__ __forceinline__ Philox4 philox4x32_10(unsigned long long counter_lo,
                                                 unsigned long long counter_hi,
                                                 unsigned long long key) {
  unsigned c0 = (unsigned)counter_lo, c1 = (unsigned)(counter_lo >> 32);
  unsigned c2 = (unsigned)counter_hi, c3 = (unsigned)(counter_hi >> 32);
  unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ Philox4 rng_next(sxmc_rng_state* st) {
  const Philox4 r = philox4x32_10(st->offset, st->subsequence, st->seed);
  st->offset += 1;
  return r;
}

// (0, 1], like curand_uniform
__device__ __forceinline__ double rng_uniform(sxmc_rng_state* st) {
  const Philox4 r = rng_next(st);
  return ((double)r.x + 1.0) * 2.3283064365386963e-10;
}

// unit normal (Box-Muller in double precision)
__device__ __forceinline__ double rng_normal(sxmc_rng_state* st) {
  const Philox4 r = rng_next(st);
  const double u1 = ((double)r.x + 1.0) * 2.3283064365386963e-10;  // (0,1]
  const double u2 = (double)r.y * 2.3283064365386963e-10;          // [0,1)
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// ------------------------------------------------------------------------------------ device parts
__device__ __forceinline__ void pick_new_vector_device(int n, sxmc_rng_state* rng,
                                                       const float* jump_width,
                                                       const double* current_vector,
                                                       double* proposed_vector) {
  const int offset = blockIdx.x * blockDim.x + threadIdx.x;
  const int stride = gridDim.x * blockDim.x;
  for (int i = offset; i < n; i += stride) {
    if (jump_width[i] > 0) {  // fixed parameters carry width -1 (mcmc.cpp:204-207)
      const double u = rng_normal(&rng[i]);
      proposed_vector[i] = current_vector[i] + jump_width[i] * u;
    } else {
      proposed_vector[i] = current_vector[i];
    }
  }
}

__device__ __forceinline__ void jump_decider_device(sxmc_rng_state* rng, double* nll_current,
                                                    const double* nll_proposed, double* v_current,
                                                    const double* v_proposed, unsigned nparameters,
                                                    int* accepted, int* counter, float* jump_buffer,
                                                    bool debug_mode) {
  const double u = rng_uniform(&rng[0]);
  const double np = nll_proposed[0];
  const double nc = nll_current[0];
  if (debug_mode || (np < nc || u <= exp(nc - np))) {  // Metropolis, nll_kernels.cpp:69-77
    nll_current[0] = np;
    for (unsigned i = 0; i < nparameters; i++) v_current[i] = v_proposed[i];
    accepted[0] += 1;
  }
  const int count = counter[0];
  for (unsigned i = 0; i < nparameters; i++) {
    jump_buffer[count * (nparameters + 1) + i] = (float)v_current[i];
  }
  jump_buffer[count * (nparameters + 1) + nparameters] = (float)nll_current[0];
  counter[0] = count + 1;
}

__device__ __forceinline__ void nll_total_device(size_t nparameters, size_t nsignals, size_t nsources,
                                                 const double* pars, const double* means,
                                                 const double* sigmas, const double* events_total,
                                                 const double* nexpected, const unsigned* n_mc,
                                                 const short* source_id, const unsigned* norms,
                                                 double* nll, const double* whitening = nullptr) {
  double sum = -events_total[0];
  if (isnan(sum)) {
    nll[0] = 1e18;
    return;
  }
  for (unsigned i = 0; i < nsignals; i++) {
    const short sid = source_id[i];
    sum += pars[sid] * nexpected[i] * norms[i] / n_mc[i];
  }
  for (unsigned i = 0; i < nparameters; i++) {
    if (i < nsources && pars[i] < 0) {  // steep penalty for negative rates
      nll[0] = 1e18;
      return;
    }
    if (sigmas[i] > 0) {
      double x = (pars[i] - means[i]) / sigmas[i];
      if (whitening != nullptr) {
        // correlated constraints (include/sxmc_hip.h, sxmc_group_set_constraint_whitening): the whitened residual
        // r_i = sum over j <= i of W_ij x_j, ascending, one fma per term, in the slot constraint i has.  This sequential
        // form keeps no vector: every x_j is formed again, by the same division.
        double r = 0.0;
        for (unsigned j = 0; j <= i; j++) {
          const double xj = sigmas[j] > 0 ? (pars[j] - means[j]) / sigmas[j] : 0.0;
          r = __fma_rn(whitening[(size_t)j * nparameters + i], xj, r);
        }
        x = r;
      }
      sum += 0.5 * x * x;
    }
  }
  nll[0] = sum;
}

// Sum of sums[0..n) over the workgroup; the total is returned to every thread.
// BD > 0: the workgroup's LOGICAL size -- the first BD lanes of a larger launch do the work of a workgroup of BD (the
// others have left): the fused step kernel runs its step-end roles in workgroups of the fill's size (see
// fill_step_kernel in pdfz_kernels.hip), and the partition of every sum must be the one a launch of BD lanes has.
template <int BD = 0>
__device__ __forceinline__ double block_sum(size_t n, const double* sums, double* s_wave /*[17]*/) {
  const unsigned bdim = BD > 0 ? (unsigned)BD : blockDim.x;
  // (a thread's terms are added in index order, as before; sixteen loads are in flight at a time -- the reference's
  //  launch shape hands 16 384 partial sums to 128 lanes, mcmc.cpp:37-45, and one load per addition made that 41 us)
  double t = 0.0;
  size_t i = threadIdx.x;
  const size_t bd = bdim;
  for (; i + 15 * bd < n; i += 16 * bd) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = sums[i + (size_t)k * bd];
#pragma unroll
    for (int k = 0; k < 16; k++) t += v[k];
  }
  for (; i < n; i += bd) t += sums[i];
  // a block size that is not a multiple of 64 leaves the last wave partly empty: what a shuffle reads from
  // a lane that does not exist is undefined, so those contributions are replaced by zero
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int live = min(kWave, (int)bdim - wave * kWave);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double o = __shfl_down(t, off, kWave);
    t += (lane + off < live) ? o : 0.0;
  }
  const int nwaves = ((int)bdim + kWave - 1) / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) s_wave[wave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < nwaves; w++) tot += s_wave[w];
    s_wave[16] = tot;
  }
  __syncthreads();
  return s_wave[16];
}

// The fused end of an MCMC step (nll_kernels.cpp:230-271): reduce the event partial sums, total the
// NLL at the proposed vector, Metropolis accept/reject + append to the jump buffer, draw the next
// proposal.  One workgroup, one launch per step, so it is built to be a few memory latencies long:
//   phase A (all lanes): everything that does not depend on the accept decision -- every input is
//     loaded once, lane j forms signal j's expected-rate term and lane i parameter i's constraint term
//     (the divisions), lane i draws its proposal deviate (lane 0 its uniform first: same consumption
//     order of generator 0 as jump_decider followed by pick_new_vector), the partial sums are reduced;
//   phase B (every lane the same, from registers filled before the sums are waited for): the terms are added in
//     the reference's order (so the value is the sequential loop's, bit for bit), accept or reject; lane 0 stores;
//   phase C (all lanes): vector copy, jump-buffer append and next proposal, one parameter per lane.
// Vectors longer than kStage fall back to the plain sequential form.
constexpr int kStage = 256;

// Returns (to every thread) whether the proposal was accepted.
// `wait`: called by every thread of the workgroup, once, after everything that does not need the partial sums has
// been loaded and computed (phase A) and before the sums are read -- the cooperative step end (step_end_kernel) waits
// there for the workgroups that are still summing, so that phase A runs under their look-ups.
// R: how many of phase B's addends every lane holds in registers across the wait and the reduction (the rest is read from
// LDS behind them): 32 -- 64 VGPRs -- in the kernels bounded at 128 lanes (the cooperative step ends) and at 256 (the
// two-launch step ends: finish_zero_kernel, finish2_zero_kernel, finish_zero_chains_kernel, eval_nll_finish_kernel, 113-115
// VGPRs in all), 8 in kernels bounded at 1024 lanes, which have 128 registers (BD > 0: the fused step; tail_step_kernel).
template <int BD = 0, int R = (BD > 0 ? 8 : 32), typename Wait>
__device__ __forceinline__ bool finish_step_device_w(size_t npartial_sums, const double* sums, size_t nsignals,
                                                     size_t nsources, const double* means, const double* sigmas,
                                                     sxmc_rng_state* rng, double* nll_current,
                                                     double* nll_proposed, double* v_current, double* v_proposed,
                                                     int* accepted, int* counter, float* jump_buffer,
                                                     int nparameters, const float* jump_width,
                                                     const double* nexpected, const unsigned* n_mc,
                                                     const short* source_id, const unsigned* norms,
                                                     const double* factor, const double* whitening,
                                                     bool debug_mode, Wait&& wait) {
  __shared__ double s_wave[17];
  __shared__ double s_vprop[kStage], s_vcur[kStage], s_z[kStage];
  __shared__ double s_d[kStage];            // with a factor: the next proposal's displacement (L z)_i, formed in phase A
                                            // (ahead of that, with a whitening matrix: the constraints' residuals x)
  __shared__ double s_add[2 * kStage];      // phase B's addends in its order: the signals' terms, then the constraints'
  __shared__ float s_jw[kStage];
  __shared__ unsigned s_badw[16];           // per wave: one of its parameters is a negative source rate
  __shared__ int s_count, s_nacc;
  __shared__ double s_nc, s_u;

  const unsigned bdim = BD > 0 ? (unsigned)BD : blockDim.x;
  const bool staged = nparameters <= kStage && nsignals <= (size_t)kStage;
  if (!staged) {   // (never with BD > 0: the host offers the fused kernel only for vectors that are staged)
    wait();
    double total_sum = block_sum<BD>(npartial_sums, sums, s_wave);
    if (threadIdx.x == 0) {
      nll_total_device(nparameters, nsignals, nsources, v_proposed, means, sigmas, &total_sum, nexpected, n_mc,
                       source_id, norms, nll_proposed, whitening);
      jump_decider_device(rng, nll_current, nll_proposed, v_current, v_proposed, nparameters, accepted, counter,
                          jump_buffer, debug_mode);
    }
    __threadfence_block();
    __syncthreads();
    // pick_new_vector over THIS workgroup's lanes (pick_new_vector_device strides over the grid: inside a launch of several
    // workgroups -- every step end of a group -- the finisher's lanes are not the grid's first, and parameters were left
    // without a proposal)
    for (int i = threadIdx.x; i < nparameters; i += (int)bdim) {
      if (jump_width[i] > 0) {  // fixed parameters carry width -1 (mcmc.cpp:204-207)
        const double u = rng_normal(&rng[i]);
        v_proposed[i] = v_current[i] + jump_width[i] * u;
      } else {
        v_proposed[i] = v_current[i];
      }
    }
    __syncthreads();
    return nll_current[0] == nll_proposed[0];   // (long vectors: accepted, or a tie, which changes nothing)
  }

  // ---- phase A
  if (threadIdx.x == 0) {
    s_nc = nll_current[0];
    s_count = counter[0];
    s_nacc = accepted[0];   // (read here, so that the accept path only stores)
  }
  double* const s_pen = s_add + nsignals;
  bool negative_rate = false;
  for (int i = threadIdx.x; i < nparameters; i += (int)bdim) {
    const double p = v_proposed[i], mean = means[i], sigma = sigmas[i];
    const float jw = jump_width[i];
    s_vprop[i] = p;
    s_vcur[i] = v_current[i];
    s_jw[i] = jw;
    // (a parameter without a constraint adds -0.0, which leaves every sum as it is, bit for bit: x + -0.0 == x for
    //  every x, both zeros and NaN included)
    double pen = -0.0;
    double x = 0.0;
    if (sigma > 0) {  // nll_kernels.cpp:181-184
      x = (p - mean) / sigma;
      pen = 0.5 * x * x;
    }
    if (whitening != nullptr) s_d[i] = x;   // (an unconstrained parameter's residual is 0: the product reads every x_j)
    if ((size_t)i < nsources && p < 0) negative_rate = true;  // :176-179
    s_pen[i] = pen;
    if (i == 0 || jw > 0) {
      sxmc_rng_state st = rng[i];
      if (i == 0) s_u = rng_uniform(&st);            // jump_decider's draw (nll_kernels.cpp:63)
      s_z[i] = (jw > 0) ? rng_normal(&st) : 0.0;     // pick_new_vector's draw (:42), free parameters only
      rng[i].offset = st.offset;
    } else if (factor != nullptr) {
      s_z[i] = 0.0;   // a fixed parameter draws nothing and its z is 0: the product below reads every z_j, j <= i
    }
  }
  for (int j = threadIdx.x; j < (int)nsignals; j += (int)bdim) {
    s_add[j] = v_proposed[source_id[j]] * nexpected[j] * norms[j] / n_mc[j];  // :169-172
  }
  const int nwaves = ((int)bdim + kWave - 1) / kWave;
  {
    const unsigned long long any_negative = __ballot(negative_rate);
    if ((threadIdx.x & (kWave - 1)) == 0) s_badw[threadIdx.x / kWave] = any_negative != 0ull ? 1u : 0u;
  }
  __syncthreads();
  // Correlated constraints (include/sxmc_hip.h, sxmc_group_set_constraint_whitening): lane i's whitened residual
  // r_i = sum over j <= i of W_ij x_j, ascending in j, one fma per term, and 0.5 r_i^2 in the slot constraint i has in
  // s_pen -- the sum below keeps its length and its order.  Here, behind the barrier that published x (in s_d, which
  // nothing else uses yet) and ahead of the wait, so that it runs under the other workgroups' event sums.  W_ij stands
  // at whitening[j * P + i]: consecutive doubles across a wave for a fixed j, x_j one LDS word for all its lanes; the
  // loads do not depend on the chain of fmas and eight are in flight at a time.  The barrier behind it completes s_pen
  // before any lane takes its addends, and lets the factor's loop reuse s_d.  The branch is uniform (a kernel argument).
  if (whitening != nullptr) {
    for (int i = threadIdx.x; i < nparameters; i += (int)bdim) {
      if (sigmas[i] > 0) {   // (an unconstrained parameter keeps its -0.0)
        const double* col = whitening + i;
        const size_t P = (size_t)nparameters;
        double r = 0.0;
        int j = 0;
        for (; j + 8 <= i + 1; j += 8) {
          double w[8];
#pragma unroll
          for (int k = 0; k < 8; k++) w[k] = col[(size_t)(j + k) * P];
#pragma unroll
          for (int k = 0; k < 8; k++) r = __fma_rn(w[k], s_d[j + k], r);
        }
        for (; j <= i; j++) r = __fma_rn(col[(size_t)j * P], s_d[j], r);
        s_pen[i] = 0.5 * r * r;
      }
    }
    __syncthreads();
  }
  // Everything phase B adds is known now.  EVERY lane takes it into registers before the wait (the first kRegAdd addends,
  // fetched together; all lanes read the same words), so that what follows the partial sums' reduction is a chain of
  // additions, the exp and the stores: no LDS round trip per addend, and no broadcast of the decision with its barrier --
  // each lane decides for itself, from the same values by the same operations, and lane 0 stores.
  constexpr int kRegAdd = R;
  static_assert(R > 0 && R % 8 == 0, "whole blocks of eight additions");
  const int nadd = (int)nsignals + nparameters;
  double add[kRegAdd];
#pragma unroll
  for (int k = 0; k < kRegAdd; k++) add[k] = s_add[min(k, max(nadd - 1, 0))];
#pragma unroll
  for (int k = 0; k < kRegAdd; k++) add[k] = k < nadd ? add[k] : -0.0;
  bool bad = false;
  for (int w = 0; w < nwaves; w++) bad = bad || s_badw[w] != 0u;
  const double nc = s_nc, u = s_u;
  const int count = s_count, nacc = s_nacc;
  // The correlated proposal (include/sxmc_hip.h, sxmc_group_set_proposal_factor): lane i's displacement d_i = sum over
  // j <= i of L_ij z_j, ascending in j, one fma per term -- here, behind the barrier that published s_z and ahead of the
  // wait, so that it runs under the event sums of the other workgroups; phase C adds it to whichever vector the decision
  // leaves.  L_ij stands at factor[j * P + i]: for a fixed j a wave's lanes read consecutive doubles, and z_j is one LDS
  // word for all of them (a broadcast).  The loads do not depend on the chain of fmas: eight are in flight at a time.
  // s_d[i] is written and read by the same lane (the same stride in phase C): no barrier of its own.
  if (factor != nullptr) {
    for (int i = threadIdx.x; i < nparameters; i += (int)bdim) {
      double d = 0.0;
      if (s_jw[i] > 0) {
        const double* col = factor + i;
        const size_t P = (size_t)nparameters;
        int j = 0;
        for (; j + 8 <= i + 1; j += 8) {
          double l[8];
#pragma unroll
          for (int k = 0; k < 8; k++) l[k] = col[(size_t)(j + k) * P];
#pragma unroll
          for (int k = 0; k < 8; k++) d = __fma_rn(l[k], s_z[j + k], d);
        }
        for (; j <= i; j++) d = __fma_rn(col[(size_t)j * P], s_z[j], d);
      }
      s_d[i] = d;
    }
  }
  wait();
  const double total_sum = block_sum<BD>(npartial_sums, sums, s_wave);  // barriers inside

  // ---- phase B: the reference's sum, term by term in its order; 1e18 on a NaN event sum or a negative source rate
  double sum = -total_sum;
  bad = bad || isnan(sum);
#pragma unroll
  for (int k0 = 0; k0 < kRegAdd; k0 += 8) {
    if (k0 < nadd) {
#pragma unroll
      for (int k = 0; k < 8; k++) sum += add[k0 + k];
    }
  }
  for (int k = kRegAdd; k < nadd; k++) sum += s_add[k];
  const double np = bad ? 1e18 : sum;
  const bool accept = debug_mode || (np < nc || u <= exp(nc - np));  // Metropolis, :69-77
  if (threadIdx.x == 0) {
    nll_proposed[0] = np;
    if (accept) {
      nll_current[0] = np;
      accepted[0] = nacc + 1;
    }
    counter[0] = count + 1;
  }

  // ---- phase C
  const double nllcur = accept ? np : nc;
  const size_t row = (size_t)count * (size_t)(nparameters + 1);
  for (int i = threadIdx.x; i < nparameters; i += (int)bdim) {
    const double cur = accept ? s_vprop[i] : s_vcur[i];
    if (accept) v_current[i] = cur;
    jump_buffer[row + i] = (float)cur;
    if (factor != nullptr) {
      v_proposed[i] = (s_jw[i] > 0) ? __dadd_rn(cur, s_d[i]) : cur;
    } else {
      v_proposed[i] = (s_jw[i] > 0) ? cur + s_jw[i] * s_z[i] : cur;  // :40-47
    }
  }
  if (threadIdx.x == 0) jump_buffer[row + nparameters] = (float)nllcur;
  return accept;
}

template <int R = 32>
__device__ __forceinline__ bool finish_step_device(size_t npartial_sums, const double* sums, size_t nsignals,
                                                   size_t nsources, const double* means, const double* sigmas,
                                                   sxmc_rng_state* rng, double* nll_current,
                                                   double* nll_proposed, double* v_current, double* v_proposed,
                                                   int* accepted, int* counter, float* jump_buffer,
                                                   int nparameters, const float* jump_width,
                                                   const double* nexpected, const unsigned* n_mc,
                                                   const short* source_id, const unsigned* norms,
                                                   const double* factor, const double* whitening,
                                                   bool debug_mode) {
  return finish_step_device_w<0, R>(npartial_sums, sums, nsignals, nsources, means, sigmas, rng, nll_current, nll_proposed,
                              v_current, v_proposed, accepted, counter, jump_buffer, nparameters, jump_width, nexpected,
                              n_mc, source_id, norms, factor, whitening, debug_mode, [] {});
}

// What the NEXT call of finish_step_device would propose if the step it decides were rejected -- i.e. from the
// vector v_current as it stands: v_current + jump_width * z with the deviates that call will draw, WITHOUT
// advancing the generators (the call itself draws them again).  Generator 0 hands the decider its uniform first.
// The look-ahead walk evaluates this vector beside the proposal (sxmc_multigroup_lookahead_step_async).
__device__ __forceinline__ void peek_next_proposal_device(int nparameters, const sxmc_rng_state* rng,
                                                          const float* jump_width, const double* v_current,
                                                          double* out) {
  for (int i = threadIdx.x; i < nparameters; i += blockDim.x) {
    const float jw = jump_width[i];
    double v = v_current[i];
    if (jw > 0) {
      sxmc_rng_state st = rng[i];
      if (i == 0) (void)rng_uniform(&st);
      v = v + jw * rng_normal(&st);
    }
    out[i] = v;
  }
}

}  // namespace sxdev
