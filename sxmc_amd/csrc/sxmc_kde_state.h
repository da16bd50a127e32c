// sxmc_kde_state.h -- what the units of the kernel-density evaluator (sxmc_kde.cpp, sxmc_kde_cv.cpp, sxmc_kde_draw.cpp)
// share: the evaluator behind sxmc_kde_t and the few functions one of them offers the others.  Internal.
#pragma once

#include "sxmc_host.h"

#include "kde_cutoff.h"
#include "kde_plan.h"

#include <memory>

static_assert(sxkde::kPlanTile == SXMC_KDE_TILE && sxkde::kPlanProjLanes == SXMC_KDE_PROJ_LANES, "kde_plan.h's geometry");

// A cutoff radius (sxmc_kde_set_cutoff): nothing of it is read at R = 0.
struct KdeCutoff {
  double cutoff = 0;               // R
  float qcut = 0;                  // sxkde::cutoff_qcut(R)
  std::shared_ptr<sxhost::DeviceBuffer<unsigned>> d_perm;   // [npad] the table rows in spatial order; one per table, shared
  sxhost::DeviceBuffer<float> d_sorted;    // [npad][rowlen()] the prepass's rows in that order (kde_cutoff_gather)
  sxhost::DeviceBuffer<float> d_tile_box;  // [npad / tile][kCutBox] the tiles' boxes of the last evaluation
  sxhost::DeviceBuffer<unsigned long long> d_visited;   // the tiles the last evaluation's waves visited: kCutCounters
                                                        // counters kCutCounterStride words apart, added on the host
  bool points_sorted = false;      // the point plan in place is the sorted one
  sxhost::DeviceBuffer<unsigned> d_inv;    // [pitch] the caller's point that stands at each sorted place
  sxhost::DeviceBuffer<float> d_wave_box;  // [pitch / 64][kCutWaveBox] the boxes of the waves of sorted points
  size_t live_waves = 0;           // waves with a live point
  unsigned long long last_possible = 0;   // live_waves * tiles of the last evaluation (0 without a lookup or a cutoff)
  bool last_cut = false;           // the last evaluation ran a lookup with a cutoff
  bool on() const { return cutoff > 0; }
};

struct sxmc_kde {
  sxmc_hist* h = nullptr;          // table, geometry, systematics and stream (one bin per observable)
  int D = 0;
  size_t nsamples = 0;
  size_t npad = 0;                 // sample rows, a multiple of SXMC_KDE_TILE
  double bw[SXMC_KDE_MAX_DIM] = {0};
  double prefactor = 0;            // 1 / ((2 pi)^(D/2) prod h)
  // what the bandwidths were made of (cross-validation scales its candidates from them: sxmc_kde_cv_select)
  double sigma[SXMC_KDE_MAX_DIM] = {0};   // standard deviation over the n_inside untransformed in-domain rows
  double scale[SXMC_KDE_MAX_DIM] = {0};   // the bandwidth scales given at creation
  size_t n_inside = 0;
  sxhost::DeviceBuffer<float> d_rows;      // [npad][D + 1]: scaled coordinates, weight; adaptive: [npad][D + 2] (rowlen())
  // adaptive bandwidths (sxmc_kde_create_adaptive): nothing of it is set or read at sensitivity 0
  double sensitivity = 0;
  sxhost::DeviceBuffer<double> d_lambda;   // [npad] the factors of the table rows, 1.0 in the padding; null when fixed
  std::vector<double> lambda;      // [nsamples] the same on the host
  // weighted Monte Carlo samples (sxmc_kde_create_weighted): nothing of it is set or read without multiplicities.  The
  // column belongs to the table: evaluators made by sxmc_kde_create_shared hold the same buffers.
  std::shared_ptr<sxhost::DeviceBuffer<unsigned>> d_mult;   // [npad] the rows' multiplicities, 0 in the padding; null: none
  std::shared_ptr<const std::vector<unsigned>> mult;        // [nsamples] the same on the host
  unsigned long long mult_total = 0;                        // their sum over ALL rows (<= 2^32 - 1)
  double n_eff = 0;                // Kish's effective sample count of the in-domain rows (n_inside without multiplicities)
  bool weighted() const { return d_mult != nullptr; }
  const unsigned* mult_ptr() const { return d_mult ? d_mult->get() : nullptr; }
  bool adaptive() const { return d_lambda.get() != nullptr; }
  int rowlen() const { return D + (adaptive() ? 2 : 1); }
  // evaluation points
  bool has_points = false;
  size_t npoints = 0, pitch = 0;
  std::vector<float> host_points;  // the caller's points as last set (a change of R plans them again)
  sxhost::DeviceBuffer<float> d_pts;       // [D][pitch] scaled coordinates (0 where the point's code is not 0); grows with d_codes
  sxhost::DeviceBuffer<int> d_codes;       // [pitch] EvalHist's point codes: 0 in domain, -1 outside, -2 another data set
  int nsplit = 1;
  unsigned tiles_per_split = 1;
  sxhost::DeviceBuffer<double> d_part;     // [nsplit][pitch] partial sums (grow-only)
  KdeCutoff cut;
  // bindings
  float* pdf = nullptr;
  int pdf_off = 0, pdf_stride = 1;
  unsigned* norm = nullptr;
  int norm_off = 0;
  const double* params = nullptr;
  int par_off = 0, par_stride = 1;
  int cus = 256;
  // streams: the evaluator's own (h->stream) carries everything but sxmc_kde_eval_on_stream_async, which launches on the
  // caller's.  ext_stream: the caller's stream of the last such launch while nothing has waited for it; own_pending:
  // work has gone to the own stream since it was last waited for.  Whoever takes the other stream next waits first
  // (order_after_caller / sxmc_kde_eval_on_stream_async).
  hipStream_t ext_stream = nullptr;
  bool ext_pending = false;
  bool own_pending = false;
  unsigned long long evaluations = 0;   // launched so far, by either entry (sxmc_kde_evaluation_count)
  // sampling (sxmc_kde_random_sample): the rows hold an evaluation once one has been launched
  bool evaluated = false;
  sxhost::DeviceBuffer<unsigned> d_flag;   // [npad] in-domain flags, then [npad] their inclusive prefix sum, then [npad] the
                                           // in-domain row numbers (one allocation, made at the first draw); with
                                           // multiplicities a draw leaves [npad] m_i of the live rows, then [npad] their
                                           // inclusive prefix sum, which the sampler searches
  sxhost::DeviceBuffer<void> d_scan_temp;
  size_t scan_temp_bytes = 0;
  // projection (sxmc_kde_project): per-row scratch, partial sums, the result and the in-domain count (grow-only)
  sxhost::DeviceBuffer<double> d_proj;
  ~sxmc_kde() { sxmc_hist_destroy(h); }   // (releases only: its buffers go by themselves, the table with its evaluator)
};

namespace sxhost {

constexpr double kLog2eHalfSqrt = 0.84932180028801907;   // sqrt(log2(e) / 2): exp(-z^2 / 2) = exp2(-(z * this)^2)
constexpr size_t kVisitedWords = (size_t)sxkde::kCutCounters * sxkde::kCutCounterStride;

// Everything but sxmc_kde_eval_on_stream_async works on the evaluator's own stream: after the last work that entry gave
// to its caller's stream.  (A host wait: these are set-up and read-out calls; not while a graph is recorded.)
int order_after_caller(sxmc_kde* k);
// The untransformed table's observables read back from the device: cols[d * nsamples + i], observable d of row i.
int table_columns(sxmc_kde* k, std::vector<float>& cols);

}  // namespace sxhost
