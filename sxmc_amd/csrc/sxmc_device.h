// sxmc_device.h -- structures shared between the host side of libsxmc_hip.so and its gfx950
// kernels.  Internal: the public boundary is include/sxmc_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/sxmc_hip.h"

#include "step_end_plan.h"   // (the step end's grids, LDS and ticket words: pure, shared with the host's rules)
#include "sxmc_device_types.h"

// Arguments of finish_nll_jump_pick_combo (nll_kernels.h:190-207) for the fused step end.
struct SxStepArgs {
  size_t nsignals, nsources;
  const double* means;
  const double* sigmas;
  sxmc_rng_state* rng;
  double* nll_current;
  double* nll_proposed;
  double* v_current;
  double* v_proposed;
  int* accepted;
  int* counter;
  float* jump_buffer;
  int nparameters;
  int debug_mode;
  const float* jump_width;
  const double* nexpected;
  const unsigned* n_mc;
  const short* source_id;
  const unsigned* norms;
  // measurement build only (the gated step): the finisher stores gate_value to *gate once the next proposal is written
  unsigned* gate = nullptr;
  unsigned gate_value = 0;
  // the correlated proposal's lower-triangular factor, P x P doubles with L_ij at [j * P + i], or null: the diagonal
  // proposal (include/sxmc_hip.h, sxmc_group_set_proposal_factor).  Staged step ends only (at most 256 parameters and
  // signals); the look-ahead pass and the lockstep sets' joint ends never get one.
  const double* factor = nullptr;
  // correlated constraints' whitening matrix, P x P doubles, lower triangular with W_ij at [j * P + i], or null: one
  // independent Gaussian per parameter (include/sxmc_hip.h, sxmc_group_set_constraint_whitening).  Staged step ends only,
  // as the factor.
  const double* whitening = nullptr;
};

// The cooperative step end's look-up pointers BY VALUE (step_end_kernel<true>): per member the two tables a worker's
// dependent loads go through -- the rows' bins, then the histogram at those bins -- as a kernel argument, so that they
// arrive in scalar registers with the launch instead of behind two more loads (the descriptor array's address, then
// fields of descriptors that span several cache lines each).  Built by the host from the same descriptors it uploads
// (sx_step_end_table_fill), wherever it uploads them; groups of more than SXMC_STEP_END_MEMBERS members keep the
// descriptor form.  Only what sits on that chain is here: 16 members x 4 scalar registers is what a wave can hold
// without spilling (a member's other fields -- normalisation, bin volume, lookup-table output -- feed the LDS staging,
// which lane j reads from descriptor j in parallel with the look-ups and needs no sooner than they land; the
// per-signal rates nexpected / n_mc / source_id are the caller's device arrays, which the library cannot see change).
#define SXMC_STEP_END_MEMBERS 16
struct SxStepEndTable {   // (entries past the last member repeat it: every entry can be addressed)
  const int* read_bins[SXMC_STEP_END_MEMBERS];    // the rows' bins (event classes, or the events themselves)
  const unsigned* bins[SXMC_STEP_END_MEMBERS];
};
inline bool sx_step_end_table_fill(SxStepEndTable& t, const SxSignalDesc* descs, size_t nsig) {
  if (nsig == 0 || nsig > SXMC_STEP_END_MEMBERS) return false;
  for (size_t u = 0; u < SXMC_STEP_END_MEMBERS; u++) {
    const SxSignalDesc& d = descs[u < nsig ? u : nsig - 1];
    t.read_bins[u] = d.read_bins;
    t.bins[u] = d.bins;
  }
  return true;
}

// The step ends of the chains of a lockstep set, launched together (sxmc_multigroup_step_async): per chain what
// eval_nll_kernel and finish_zero_kernel take.  Passed by value (kernel argument); the chain is blockIdx.y.
#define SXMC_MAX_LOCKSTEP 4
struct SxChainEnd {
  const SxSignalDesc* lookup_descs;  // the rows the event sum runs over (event classes, or the events themselves)
  const SxSignalDesc* hist_descs;    // the chain's histograms and normalisations (cleared for the next evaluation)
  unsigned long long nrows;
  const unsigned* weight;            // events per row, or null
  double* sums;                      // nblocks partial event sums
  unsigned* ticket;
  unsigned nblocks;                  // workgroups of this chain's event sum (step_sum_blocks: as in its sequential step)
  SxStepArgs a;
};
struct SxChainEnds {
  SxChainEnd c[SXMC_MAX_LOCKSTEP];
};

// Host-callable launchers implemented in the .hip files -------------------------------------
struct SxLaunchShape {
  int nobs;
  int nslot;
  int lds_hist;     // 1: LDS-privatized sub-histograms, 0: global atomics into the HBM histogram
  int threads;      // 256 / 512 / 1024
  int grid;
  size_t lds_bytes;
  int debug_mode;   // measurement hook, see fill_kernel
  int static_prog;  // index into the static program table, or -1: decode the program at run time
  void* rtc_fill;   // kernel specialised at run time for this launch (hipFunction_t), or null: built-in kernels
  void* rtc_sparse; // ... and for its sparse flavour over runs
  int sparse_runs;  // 1: the sparse flavour of this launch runs fill_sparse_kernel (bucketed table laid out in runs)
  size_t sparse_lds_bytes;
  unsigned lds_layout;  // ordered / boxed forms: words between the LDS histogram's replicas | log2(replicas) << 24
                        // (boxed: always the padded form with queues)
  int form;         // the table's form (kForm*, sxmc_device_types.h); static_prog indexes the programs built in for it
  // profiling (sxmc_group_profile): when set, the fill is launched through hipExtLaunchKernelGGL /
  // hipExtModuleLaunchKernel with these two HIP events, which then carry the DISPATCH's own begin and end timestamps
  // -- the kernel's duration as rocprofv3 --kernel-trace reports it.  (Two hipEventRecord calls around the launch
  // also time the packets between them: +2.5-3 us per launch, a fifth of BASELINE config 2's fill.)
  void* ev_start = nullptr;
  void* ev_stop = nullptr;
  // the whole step in this launch (fill_step_kernel): HOST image of the step end's arguments (sx_tail_args_fill; passed
  // to the kernel by value) and the extra workgroups (finisher + workers) appended to the grid; null: the fill alone
  const void* tail = nullptr;
  int tail_blocks = 0;
  // the members carry sample multiplicities (sxmc_hist_set_sample_multiplicities): fill_kernel<..., kPreWeighted> over the rows
  // form, its one built-in program (static_prog >= 0: sx_fill_weighted_supports), else the program decoded at run time or the
  // shape-agnostic kernel; no run-time specialisation, no form fused with the step end
  int weighted = 0;
};
bool sx_fill_has_step_form(const SxLaunchShape& sh);
// The fill kernels' `w` argument: the replica layout (ordered / boxed forms), else the histogram words the launch's LDS
// holds beside its 4 header words and, with the histogram in LDS, 64 trash words.
inline unsigned sx_fill_w(const SxLaunchShape& sh) {
  return sx_form_ordered(sh.form) ? sh.lds_layout : (unsigned)(sh.lds_bytes / 4 - 4 - (sh.lds_hist ? 64 : 0));
}
size_t sx_tail_args_bytes();
void sx_tail_args_fill(void* image, const SxSignalDesc* lookup_descs, const SxSignalDesc* hist_descs, int nsig,
                       int max_bins, unsigned long long npoints, const unsigned* weight, const double* real_weight,
                       unsigned long long* slots, double* last_good, unsigned* sync, int nvb, const struct SxStepArgs& a);
// (real_weight: real event weights in `weight`'s place -- the roles' double instantiation; null: counts, or neither)

// A fill kernel specialised at run time (sxmc_rtc.cpp): the template arguments of fill_body / fill_sparse_body.
struct SxRtcSpec {
  int nobs, nslot, lds_hist, form, sparse_runs;
  int nchain;                    // > 1: the lockstep-chains kernel (fill_multi_body), histograms in LDS
  int max_threads;               // launch bound of the kernel (0 = 1024): several chains over an ordered table need more
                                 // registers than 1024 lanes leave (spills inside the stream loop: every reload drains
                                 // the loads in flight), so their kernels are compiled for the workgroup they get
  int nops;
  unsigned ops[SXMC_MAX_SYST];   // type | obs_slot << 4 | extra_slot << 8 | npars << 12 (0 = one coefficient)
};
bool sx_rtc_compile_only(const SxRtcSpec& k, size_t* code_bytes, std::string* err);
void* sx_rtc_get(const SxRtcSpec& k, std::string* err);
struct SxChainDescsHost {
  const SxSignalDesc* d[4];
};
hipError_t sx_rtc_launch_multi(void* fn, int grid, int threads, size_t lds_bytes, const SxChainDescsHost& chains,
                               const SxSegment* segs, const unsigned* blk_off, unsigned hist_words, unsigned dbg,
                               hipStream_t s, void* ev_start = nullptr, void* ev_stop = nullptr);
hipError_t sx_rtc_launch(void* fn, int grid, int threads, size_t lds_bytes, const SxSignalDesc* descs,
                         const SxSegment* segs, const unsigned* blk_off, unsigned w, unsigned dbg, hipStream_t s,
                         void* ev_start = nullptr, void* ev_stop = nullptr);

hipError_t sx_launch_zero(const SxSignalDesc* d_descs, int nsig, int max_bins, unsigned* ticket, hipStream_t s);
// (the launchers of a row sum are templates over the row weight's type W: unsigned counts -- null: none --, or double
//  event weights; both instantiated in pdfz_kernels.hip's unit)
template <typename W>
hipError_t sx_launch_step_end(const SxSignalDesc* lookup_descs, const SxSignalDesc* hist_descs, int nsig, int max_bins,
                              unsigned long long npoints, const W* weight, unsigned long long* slots,
                              double* last_good, unsigned* sync, int nvb, const SxStepArgs& a, hipStream_t s,
                              const SxStepEndTable* table = nullptr);   // (the lookup members by value, or null)
hipError_t sx_launch_step_end2(const SxSignalDesc* lookup_a, const SxSignalDesc* lookup_b, const SxSignalDesc* hist_a,
                               const SxSignalDesc* hist_b, int nsig, int max_bins, unsigned long long npoints,
                               const unsigned* weight_a, const unsigned* weight_b, unsigned long long* slots,
                               double* last_good, unsigned* sync, int nvb, const unsigned* norms_b, double* v_b,
                               const int* cap, const SxStepArgs& a, hipStream_t s);
hipError_t sx_step_end_slots_init(unsigned long long* slots, double* last_good, int n);
int sx_step_end_resident_capacity(int nsig, int cus);
hipError_t sx_launch_chain_ends(const SxChainEnds& e, int nchains, int nsig, int max_bins, int block, hipStream_t s);
hipError_t sx_launch_finish_zero(const SxSignalDesc* d_descs, int nsig, int max_bins, size_t npartial,
                                 const double* sums, unsigned* ticket, const SxStepArgs& a, int block, hipStream_t s);
template <typename W>
hipError_t sx_launch_eval_nll_finish(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                                      const W* weight, double* sums, unsigned* ticket, const SxStepArgs& a,
                                      int grid, int block, hipStream_t s);
hipError_t sx_launch_eval_nll2(const SxSignalDesc* descs_a, const SxSignalDesc* descs_b, int nsig,
                               unsigned long long npoints, const unsigned* weight_a, const unsigned* weight_b,
                               const double* pars_a, const double* pars_b, const double* nexpected,
                               const unsigned* n_mc, const short* source_id, const unsigned* norms_a,
                               const unsigned* norms_b, double* sums_a, double* sums_b, int half, int block,
                               hipStream_t s);
hipError_t sx_launch_finish2_zero(const SxSignalDesc* descs_a, const SxSignalDesc* descs_b, int nsig, int max_bins,
                                  size_t npartial, const double* sums_a, const double* sums_b, const unsigned* norms_b,
                                  double* v_b, const int* cap, const SxStepArgs& a, int block, hipStream_t s);
hipError_t sx_launch_peek_next_proposal(int nparameters, const sxmc_rng_state* rng, const float* jump_width,
                                        const double* v_current, double* out, hipStream_t s);
template <typename W>
hipError_t sx_launch_tail_step(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                               const W* weight, const SxStepArgs& a, hipStream_t s);
hipError_t sx_launch_fill(const SxLaunchShape& shape, const SxSignalDesc* d_descs, const SxSegment* d_segs,
                          const unsigned* d_blk_off, hipStream_t s);
hipError_t sx_launch_fill_sparse_runs(const SxLaunchShape& shape, const SxSignalDesc* d_descs, const SxSegment* d_segs,
                                      const unsigned* d_blk_off, hipStream_t s);
bool sx_fill_has_specialization(int nobs, int nslot);
// The programs built in: the index of the one for this form of table and compacted problem, or -1; and whether program
// `prog` has a kernel for this form and histogram mode (sparse_runs: the event-bin counters over a bucketed table's runs).
int sx_fill_find_program(int form, int nobs, int nslot, int nops, const unsigned* ops);
bool sx_fill_supports(int prog, int form, int lds_hist, int sparse_runs);
// Has the WEIGHTED fill (fill_body with PREW = kPreWeighted, rows form) a straight-line kernel for built-in program `prog`?
// (The registry says: one has, BASELINE config 3's.)  Otherwise a weighted launch decodes its program at run time.
bool sx_fill_weighted_supports(int prog, int lds_hist);
hipError_t sx_launch_prebin(const SxSignalDesc* d_desc, unsigned long long npad, unsigned mask, int width, void* out,
                            hipStream_t s);
// bucketed copy of a sample table (layout_kernels.hip)
hipError_t sx_bucket_keys(const SxSignalDesc* d_desc, unsigned long long nsamples, unsigned mask, const unsigned* radix,
                          unsigned outside, const unsigned* d_rows_in, unsigned* d_keys, unsigned* d_rows,
                          hipStream_t s);
hipError_t sx_order_keys(const float* d_col, unsigned long long nsamples, unsigned* d_keys, unsigned* d_rows,
                         hipStream_t s);
hipError_t sx_bucket_edges(const float* d_col, const unsigned* d_valid, unsigned long long ngranules, float* d_edges,
                           hipStream_t s);
// boxed observable (fill_boxed_kernel): sort keys by (stratum of x - t, x); per-granule boxes; one column as u16 codes
hipError_t sx_box_keys(const float* d_colx, const float* d_colt, unsigned long long nsamples, int pass, int nstrata,
                       const unsigned* bounds, unsigned* d_keys, unsigned* d_rows, hipStream_t s);
hipError_t sx_bucket_boxes(const float* d_colx, const float* d_colt, const unsigned* d_valid, unsigned long long ngranules,
                           float* d_boxes, hipStream_t s);
hipError_t sx_column_codes16(const float* col, double base, double step, unsigned long long n, unsigned short* qcol,
                             unsigned long long* tally, hipStream_t s);
hipError_t sx_bucket_sort(const unsigned* keys_in, unsigned* keys_out, const unsigned* rows_in, unsigned* rows_out,
                          unsigned long long n, int bits, hipStream_t s);
hipError_t sx_bucket_first(const unsigned* sorted_keys, unsigned long long n, unsigned* d_first, hipStream_t s);
hipError_t sx_bucket_gather(const float* cols, unsigned long long pitch, int ncols, const int* col_list,
                            const unsigned* sorted_rows, const unsigned* d_src, const unsigned* d_valid,
                            unsigned long long ngranules, float* out, unsigned long long out_pitch, hipStream_t s);
// 16-bit codes of the streamed columns of a bucketed copy (fill_ordered_body's CODES)
hipError_t sx_column_minmax(const float* cols, unsigned long long pitch, int ncols, unsigned long long n, float* out,
                            hipStream_t s);
hipError_t sx_column_codes(const float* cols, unsigned long long pitch, int nslots, const double* base, const double* step,
                           unsigned long long n, unsigned* qcol, unsigned long long* tally, hipStream_t s);
hipError_t sx_hist_cdf(const unsigned* d_bins, unsigned* d_cdf, int nbins_total, hipStream_t s);
hipError_t sx_random_sample(const unsigned* d_cdf, int nbins_total, int nobs, const int* nbins, const double* lower,
                            const double* upper, const double* scale, const float* cut_lo, const float* cut_hi,
                            unsigned long long seed, unsigned long long n, float dataset, float* d_out,
                            unsigned* d_exhausted, hipStream_t s);
// the marginal of a histogram along one observable (project_kernels.hip): d_out[0 .. nb) 64-bit totals, zero on entry
hipError_t sx_hist_project(const unsigned* d_bins, unsigned long long total, unsigned stride, unsigned nb,
                           unsigned long long* d_out, unsigned max_blocks, hipStream_t s);
hipError_t sx_launch_eval_pdf(const SxSignalDesc* d_descs, int nsig, unsigned long long max_points,
                              hipStream_t s);
template <typename W>
hipError_t sx_launch_eval_nll(const SxSignalDesc* d_descs, int nsig, unsigned long long npoints,
                              const W* weight, const double* pars, const double* nexpected, const unsigned* n_mc,
                              const short* source_id, const unsigned* norms, double* sums,
                              int grid, int block, hipStream_t s);
// The event sum over a mixed table (columns_kernels.hip): d_member_of[j] >= 0: column j is looked up from that member of
// d_descs; -1: column j of lut (ne floats at lut + j * ne).  block <= 256.  Writes sums[0 .. grid * block).
hipError_t sx_launch_nll_columns(const SxSignalDesc* d_descs, const int* d_member_of, int nsignals, const float* lut,
                                 unsigned long long ne, const double* pars, const double* nexpected,
                                 const unsigned* n_mc, const short* source_id, const unsigned* norms, double* sums,
                                 int grid, int block, hipStream_t s);
hipError_t sx_launch_pow_int(const double* x, int n, int i, double* out, hipStream_t s);
hipError_t sx_launch_transpose(const float* aos, float* cols, unsigned long long nsamples,
                               int nfields, unsigned long long col_pitch, hipStream_t s);
hipError_t sx_launch_untranspose_obs(const float* cols, float* out, unsigned long long nsamples,
                                     int nobs, unsigned long long col_pitch, float dataset,
                                     hipStream_t s);

// pdfz::EvalKernel (kde_kernels.hip; sxmc_kde.cpp, sxmc_kde_cv.cpp, sxmc_kde_draw.cpp)
#define SXMC_KDE_MAX_DIM 4   // observables of a kernel-density evaluator
#define SXMC_KDE_TILE 256    // samples per f32 partial sum of the pair kernel; sample rows are padded to a multiple
// The prepass's geometry: rows = [npad][nobs + 1] floats (scaled coordinates, weight), norm = the in-domain counter.
struct SxKdeArgs {
  float* rows;
  unsigned long long npad;
  unsigned* norm;
  double lower[SXMC_KDE_MAX_DIM];
  double upper[SXMC_KDE_MAX_DIM];
  double cscale[SXMC_KDE_MAX_DIM];       // sqrt(log2(e) / 2) / h
  double inv_h_sqrt2[SXMC_KDE_MAX_DIM];  // 1 / (h sqrt 2)
  // an adaptive evaluator's factors, [npad] (1.0 in the padding), or null.  With them the rows are D + 2 floats: the
  // same coordinates, 1 / lambda^2 and weight / lambda^D, the mass taken at h lambda.
  const double* lambda;
};
// mult: [npad] the rows' multiplicities, 0 in the padding (sxmc_kde_create_weighted: a row counts m_i in the norm and
// its weight is m_i / mass), or null: the kernels of an evaluator without them.
hipError_t sx_kde_prepass(const SxSignalDesc& d, const SxKdeArgs& a, const unsigned* mult, hipStream_t s);
// pts: [D][pitch] scaled point coordinates, pitch a multiple of 256; part: [nsplit][pitch]; adaptive: rows of D + 2
// floats (an adaptive evaluator's prepass)
hipError_t sx_kde_pairs(int D, bool adaptive, const float* pts, unsigned long long pitch, const float* rows,
                        unsigned tiles_per_split, unsigned ntiles, int nsplit, double* part, hipStream_t s);
// order: null (the partial sums stand in the caller's point order), or [npoints] the caller's point that stands at each
// sorted place (a cutoff); codes: in the caller's order
hipError_t sx_kde_combine(const double* part, unsigned long long pitch, int nsplit, unsigned long long npoints,
                          const int* codes, const unsigned* order, const unsigned* norm, double prefactor, float* out,
                          long stride, hipStream_t s);
// The cutoff radius (sxmc_kde_set_cutoff; kde_cutoff.h has the pure parts).  perm: [ntiles * 256] a permutation of the
// sample rows; sorted: the rows in that order; box: [ntiles][sxkde::kCutBox] the tiles' boxes, written by the gather.
hipError_t sx_kde_cutoff_gather(int D, bool adaptive, const float* rows, const unsigned* perm, unsigned ntiles,
                                float* sorted, float* box, hipStream_t s);
// pts: the sorted points; wave_box: [pitch / 64][sxkde::kCutWaveBox]; visited: the tiles visited, added to --
// sxkde::kCutCounters counters, sxkde::kCutCounterStride 64-bit words apart.
hipError_t sx_kde_pairs_cutoff(int D, bool adaptive, const float* pts, unsigned long long pitch, const float* rows,
                               const float* tile_box, const float* wave_box, unsigned tiles_per_split, unsigned ntiles,
                               int nsplit, float qcut, double* part, unsigned long long* visited, hipStream_t s);
// Sampling from the last evaluation (sxmc_kde_random_sample): the in-domain rows listed by a flag, an inclusive scan
// (temp: the scan's scratch, temp_bytes of it) and a scatter into idx; then one lane per event.
struct SxKdeSampleArgs {
  double lower[SXMC_KDE_MAX_DIM];
  double upper[SXMC_KDE_MAX_DIM];
  double h[SXMC_KDE_MAX_DIM];            // bandwidths
  double inv_cscale[SXMC_KDE_MAX_DIM];   // h / sqrt(log2(e) / 2): scaled row coordinate -> x - lower
  float bottom[SXMC_KDE_MAX_DIM];        // the smallest float >= lower
  float top[SXMC_KDE_MAX_DIM];           // the largest float < upper
  float cut_lo[SXMC_KDE_MAX_DIM];
  float cut_hi[SXMC_KDE_MAX_DIM];
  int has_cuts;
  float dataset;
};
// rowlen: floats to a sample row, the weight last.
hipError_t sx_kde_compact(const float* rows, int rowlen, unsigned long long npad, unsigned* flag, unsigned* pos,
                          unsigned* idx, void* temp, size_t temp_bytes, hipStream_t s);
// inclusive prefix sum of n unsigned (layout_kernels.hip); temp == nullptr: temp_bytes receives the scratch it needs
hipError_t sx_inclusive_sum_u32(const unsigned* d_in, unsigned* d_out, int n, void* temp, size_t& temp_bytes,
                                hipStream_t s);
// lambda: an adaptive evaluator's factors per table row (rows of D + 2 floats then), or null (rows of D + 1).
hipError_t sx_kde_sample(int D, const float* rows, const double* lambda, const unsigned* idx, unsigned n,
                         const SxKdeSampleArgs& g, unsigned long long seed, unsigned long long nevents, float* out,
                         unsigned* exhausted, hipStream_t s);
// ... over weighted samples: cum = the inclusive prefix sum over all npad rows of m_i where the last evaluation left
// row i a weight > 0 (flag: scratch, [npad]); total = cum[npad - 1] > 0; an event's first word picks
// target = (word * total) >> 32 and the first row whose cum exceeds it.
hipError_t sx_kde_weighted_scan(const float* rows, int rowlen, unsigned long long npad, const unsigned* mult,
                                unsigned* flag, unsigned* cum, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t sx_kde_sample_weighted(int D, const float* rows, const double* lambda, const unsigned* cum, unsigned total,
                                  unsigned long long npad, const SxKdeSampleArgs& g, unsigned long long seed,
                                  unsigned long long nevents, float* out, unsigned* exhausted, hipStream_t s);
// Projection onto one observable (sxmc_kde_project; the arithmetic is written out in include/sxmc_hip.h).  scratch:
// [2 npad] doubles (u and the reciprocal mass of every sample row), then [nsplit][pitch] partial sums, pitch = the bins
// rounded up to SXMC_KDE_PROJ_LANES; count: the in-domain rows, zero on entry.  rows_per_split sample rows to a
// workgroup, whatever the device, and the splits are added in their order: the same bits everywhere.
#define SXMC_KDE_PROJ_LANES 64
struct SxKdeProjectArgs {
  int D, obs, nbins;
  unsigned long long npad;
  unsigned rows_per_split, nsplit;
  unsigned long long pitch;
  double lower, upper;      // of the observable
  double h;                 // its bandwidth
  double cunit;             // sqrt(log2(e) / 2): a row's coordinate is (s - lower) / h times this
  const double* lambda;     // an adaptive evaluator's factors, [npad], or null.  With them rows are D + 2 floats and
                            // the per-row scratch is [3 npad]: u, the reciprocal mass at h lambda, 1 / lambda
};
// mult: [npad] the rows' multiplicities (a live row's reciprocal mass times m_i, the count their sum), or null.
hipError_t sx_kde_project(const float* rows, const SxKdeProjectArgs& a, const unsigned* mult, double* scratch,
                          unsigned* count, double* d_prob, hipStream_t s);
// The pilot of an adaptive evaluator (sxmc_kde_create_adaptive): the fixed-bandwidth PDF at zero systematics at every
// table row, in f64.  x: [D][pitch] the rows' observables (pitch a multiple of 256, padded with anything finite);
// s0: [n][D + 1] the in-domain samples and their truncation weights, in table order; part: [nsplit][pitch];
// f: [pitch] the result.  per_split samples to a workgroup, set from n alone; the splits are added in their order.
struct SxKdePilotArgs {
  int D;
  unsigned long long pitch;
  unsigned long long n;
  unsigned per_split, nsplit;
  double h[SXMC_KDE_MAX_DIM];
  double prefactor;         // 1 / ((2 pi)^(D/2) prod h)
};
// total: 0, or (weighted samples: s0's weights are m_j / mass_j) the multiplicities' total S1, which then divides in
// place of n.
hipError_t sx_kde_pilot(const SxKdePilotArgs& a, const double* x, const double* s0, double total, double* part,
                        double* f, hipStream_t s);
// One scan of likelihood cross-validation (sxmc_kde_cv_scores): K candidate bandwidth vectors scored on m rows in one
// pass over the pairs.  KP: K rounded up to a count the pair kernel is built for (sx_kde_cv_padded; the padding weighs
// 0).  x: [D][pitch] the m rows' observables (pitch a multiple of 256, zeros beyond m); s0: [m][D + KP] per sample its
// D observables, then (written by the scan itself) its KP weights 1 / prod_d (h_cd M_jd); cand: [KP][D] g_cd =
// 1 / (2 h_cd^2), then [KP][D] 1 / (h_cd sqrt 2), then [KP] prod_d h_cd; part: [nsplit][KP][pitch];
// lnf: [K][pitch] the result, ln f_-i per candidate and row.  per_split rows to a workgroup, set from m and K alone.
#define SXMC_KDE_CV_MAX 32
struct SxKdeCvArgs {
  int D, K, KP;
  unsigned m;
  unsigned long long pitch;
  unsigned per_split, nsplit;
  double lower[SXMC_KDE_MAX_DIM];
  double upper[SXMC_KDE_MAX_DIM];
  double prefactor;         // 1 / ((2 pi)^(D/2) (m - 1))
};
int sx_kde_cv_padded(int K);
hipError_t sx_kde_cv_scan(const SxKdeCvArgs& a, const double* x, double* s0, const double* cand, double* part,
                          double* lnf, hipStream_t s);
