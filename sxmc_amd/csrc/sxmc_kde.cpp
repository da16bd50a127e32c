// sxmc_kde.cpp -- the evaluator behind pdfz::EvalKernel (sxmc_kde_*): the kernel-density PDF.  The contract is written
// out in include/sxmc_hip.h and sxmc_amd/include/sxmc/pdfz.h; the kernels are in kde_kernels.hip.
//
// The sample table, the constructor's validation and the systematics are an EvalHist's: the evaluator holds an
// internal histogram evaluator with one bin per observable that is never evaluated itself -- it uploads the table
// column-major, checks and packs the systematics, and gives the fill's descriptor (fill_desc), which the prepass reads
// with the fill's own arithmetic.  So the norm is the histogram's, bit for bit.
//
// Adaptive bandwidths (sxmc_kde_create_adaptive, sensitivity > 0): the factors lambda of the table rows are fixed at
// creation -- the pilot on the device, g and lambda on the host (kde_adaptive.h) -- and kept in d_lambda; with them the
// rows are D + 2 floats and every launch takes its adaptive form.  At sensitivity 0 d_lambda is null and every launch
// is the fixed-bandwidth one.
//
// Cross-validation (sxmc_kde_cv_scores, sxmc_kde_cv_select; the host arithmetic in kde_cv.h): the untransformed in-domain
// rows are read back from the table, the candidates' constants made on the host, the weights, the pair sums and the
// logarithms on the device (kde_cv_* of kde_kernels.hip), the m logarithms of a candidate added here in table order.
// The evaluator keeps sigma, its scales and the in-domain count from creation for it; its bandwidths never change.
//
// A cutoff radius (sxmc_kde_set_cutoff; the pure parts in kde_cutoff.h): the spatial order of the table rows is made on
// the host when a cutoff is first set and kept on the device (shared evaluators hold the same buffer); the points are
// planned in the same order by set_eval_points, which keeps the caller's points so that a change of R can plan them
// again.  Everything an evaluation needs is allocated there: kde_launch allocates nothing.  At R = 0 the launches are
// the ones above and the points stay in the caller's order.
#include "sxmc_host.h"

#include "kde_adaptive.h"
#include "kde_cutoff.h"
#include "kde_cv.h"

#include <limits>
#include <memory>

using namespace sxhost;

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
  DeviceBuffer<float> d_rows;      // [npad][D + 1]: scaled coordinates, weight; adaptive: [npad][D + 2] (rowlen())
  // adaptive bandwidths (sxmc_kde_create_adaptive): nothing of it is set or read at sensitivity 0
  double sensitivity = 0;
  DeviceBuffer<double> d_lambda;   // [npad] the factors of the table rows, 1.0 in the padding; null when fixed
  std::vector<double> lambda;      // [nsamples] the same on the host
  int rowlen() const { return D + (d_lambda ? 2 : 1); }
  // evaluation points
  bool has_points = false;
  size_t npoints = 0, pitch = 0;
  DeviceBuffer<float> d_pts;       // [D][pitch] scaled coordinates (0 where the point's code is not 0); grows with d_codes
  DeviceBuffer<int> d_codes;       // [pitch] EvalHist's point codes: 0 in domain, -1 outside, -2 another data set
  int nsplit = 1;
  unsigned tiles_per_split = 1;
  DeviceBuffer<double> d_part;     // [nsplit][pitch] partial sums (grow-only)
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
  DeviceBuffer<unsigned> d_flag;   // [npad] in-domain flags, then [npad] their inclusive prefix sum, then [npad] the
                                   // in-domain row numbers (one allocation, made at the first draw)
  DeviceBuffer<void> d_scan_temp;
  size_t scan_temp_bytes = 0;
  // cutoff radius (sxmc_kde_set_cutoff): nothing of it is read at R = 0
  double cutoff = 0;               // R
  float qcut = 0;                  // sxkde::cutoff_qcut(R)
  std::shared_ptr<DeviceBuffer<unsigned>> d_perm;   // [npad] the table rows in spatial order; one per table, shared
  DeviceBuffer<float> d_sorted;    // [npad][rowlen()] the prepass's rows in that order (kde_cutoff_gather)
  DeviceBuffer<float> d_tile_box;  // [npad / tile][kCutBox] the tiles' boxes of the last evaluation
  DeviceBuffer<unsigned long long> d_visited;   // the tiles the last evaluation's waves visited: kCutCounters
                                                // counters kCutCounterStride words apart, added on the host
  std::vector<float> host_points;  // the caller's points as last set (a change of R plans them again)
  bool points_sorted = false;      // the point plan in place is the sorted one
  DeviceBuffer<unsigned> d_inv;    // [pitch] the caller's point that stands at each sorted place
  DeviceBuffer<float> d_wave_box;  // [pitch / 64][kCutWaveBox] the boxes of the waves of sorted points
  size_t live_waves = 0;           // waves with a live point
  unsigned long long last_possible = 0;   // live_waves * tiles of the last evaluation (0 without a lookup or a cutoff)
  bool last_cut = false;           // the last evaluation ran a lookup with a cutoff
  // projection (sxmc_kde_project): per-row scratch, partial sums, the result and the in-domain count (grow-only)
  DeviceBuffer<double> d_proj;
  ~sxmc_kde() { sxmc_hist_destroy(h); }   // (releases only: its buffers go by themselves, the table with its evaluator)
};

namespace {

constexpr double kLog2eHalfSqrt = 0.84932180028801907;   // sqrt(log2(e) / 2): exp(-z^2 / 2) = exp2(-(z * this)^2)

// How the pair sum is split over workgroups: s splits of the sample tiles, each a workgroup per 256 points.  Of the
// splits that keep every workgroup's share whole, the one with the fewest rounds of `slots` resident workgroups times
// tiles per workgroup (the smallest on a tie).
void choose_split(size_t pitch, size_t ntiles, int cus, int& nsplit, unsigned& tiles_per_split) {
  const unsigned long long pblocks = pitch / 256, slots = (unsigned long long)cus * 8;
  unsigned long long best = ~0ull;
  nsplit = 1;
  tiles_per_split = (unsigned)ntiles;
  const unsigned long long smax = std::min<unsigned long long>(ntiles, std::max<unsigned long long>(1, 64 * slots / pblocks));
  for (unsigned long long s = 1; s <= smax; s++) {
    const unsigned long long tps = (ntiles + s - 1) / s;
    const unsigned long long used = (ntiles + tps - 1) / tps;
    const unsigned long long cost = (pblocks * used + slots - 1) / slots * tps;
    if (cost < best) {
      best = cost;
      nsplit = (int)used;
      tiles_per_split = (unsigned)tps;
    }
  }
}

// Everything but sxmc_kde_eval_on_stream_async works on the evaluator's own stream: after the last work that entry gave
// to its caller's stream.  (A host wait: these are set-up and read-out calls; not while a graph is recorded.)
int order_after_caller(sxmc_kde* k) {
  if (!k->ext_pending) return SXMC_OK;
  if (t_capturing) return fail(SXMC_ERR_STATE, "EvalKernel: not while recording a graph");
  // (a caller that destroyed its stream without an eval_finished in between: the runtime refuses the handle, and the
  // device-wide wait covers whatever that stream still carried)
  if (hipStreamSynchronize(k->ext_stream) != hipSuccess) {
    (void)hipGetLastError();
    SX_HIP(hipDeviceSynchronize());
  }
  k->ext_pending = false;
  return SXMC_OK;
}

// The cleared sample rows of a new evaluator that has its table (k->h) and npad.
int cleared_rows(sxmc_kde* k) {
  const size_t n = k->npad * (size_t)k->rowlen();
  SX_BUF(k->d_rows.alloc(n));
  SX_HIP(hipMemset(k->d_rows.get(), 0, sizeof(float) * n));
  return SXMC_OK;
}

constexpr size_t kVisitedWords = (size_t)sxkde::kCutCounters * sxkde::kCutCounterStride;

// What an evaluation with a cutoff writes besides the rows: allocated once, cleared.
int cutoff_buffers(sxmc_kde* k) {
  const size_t ntiles = k->npad / SXMC_KDE_TILE;
  if (!k->d_sorted.get()) {
    const size_t n = k->npad * (size_t)k->rowlen();
    SX_BUF(k->d_sorted.alloc(n));
    SX_HIP(hipMemset(k->d_sorted.get(), 0, sizeof(float) * n));
  }
  if (!k->d_tile_box.get()) {
    std::vector<float> box(ntiles * (size_t)sxkde::kCutBox, 1.0f);
    for (size_t t = 0; t < ntiles; t++) sxkde::cutoff_empty_box(&box[t * sxkde::kCutBox], &box[t * sxkde::kCutBox + sxkde::kCutMaxDim]);
    SX_BUF(k->d_tile_box.alloc(box.size()));
    SX_HIP(hipMemcpy(k->d_tile_box.get(), box.data(), sizeof(float) * box.size(), hipMemcpyHostToDevice));
  }
  if (!k->d_visited.get()) {
    SX_BUF(k->d_visited.alloc(kVisitedWords));
    SX_HIP(hipMemset(k->d_visited.get(), 0, sizeof(unsigned long long) * kVisitedWords));
  }
  return SXMC_OK;
}

// The spatial order of the table rows (kde_cutoff.h), from the untransformed table read back, onto the device.
int cutoff_sample_order(sxmc_kde* k) {
  const int D = k->D;
  const size_t n = k->nsamples;
  SX_REQUIRE(k->npad <= 0xFFFFFFFFull, "EvalKernel: too many samples for a cutoff");
  std::vector<float> cols((size_t)D * n), x((size_t)D * n);
  for (int d = 0; d < D && n; d++) {   // (column d of the column-major table is observable d)
    SX_HIP(hipMemcpy(cols.data() + (size_t)d * n, k->h->store->d_cols.get() + (size_t)d * k->h->pitch, sizeof(float) * n,
                     hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < n; i++) {
    for (int d = 0; d < D; d++) x[i * (size_t)D + (size_t)d] = cols[(size_t)d * n + i];
  }
  const std::vector<uint32_t> order = sxkde::cutoff_sample_order(D, x.data(), (size_t)D, n, k->npad, k->h->lower.data(),
                                                                 k->h->upper.data());
  auto perm = std::make_shared<DeviceBuffer<unsigned>>();
  SX_BUF(perm->alloc(k->npad));
  SX_HIP(hipMemcpy(perm->get(), order.data(), sizeof(unsigned) * k->npad, hipMemcpyHostToDevice));
  k->d_perm = perm;
  return SXMC_OK;
}

// The points of k->host_points onto the device, in the caller's order (R = 0) or sorted with the waves' boxes and the
// permutation (R > 0).  The evaluator is idle.
int plan_points(sxmc_kde* k) {
  const int D = k->D;
  const size_t row = (size_t)D + 1;
  const float* points = k->host_points.data();
  const size_t n = k->host_points.size() / row;
  // EvalHist's point codes (pdfz.cpp:264-301) with one bin of zero scale per observable: every point inside the
  // domain of this data set lands in bin 0
  const std::vector<double> zero((size_t)D, 0.0);
  const std::vector<int> unit((size_t)D, 1);
  std::vector<int> codes;
  sxplan::eval_point_bins(points, n, D, k->h->lower.data(), k->h->upper.data(), zero.data(), unit.data(), 1,
                          k->h->dataset, codes);
  const size_t pitch = std::max<size_t>(256, (n + 255) / 256 * 256);
  const bool sorted = k->cutoff > 0;
  std::vector<uint32_t> order;   // (sorted) the point that stands at each sorted place
  size_t nlive = 0;
  if (sorted) order = sxkde::cutoff_point_order(D, points, n, codes.data(), k->h->lower.data(), k->h->upper.data(), &nlive);
  std::vector<float> pts(pitch * (size_t)D, 0.0f);
  for (size_t j = 0; j < n; j++) {
    const size_t i = sorted ? order[j] : j;
    if (codes[i] != 0) continue;
    for (int d = 0; d < D; d++) {
      const double c = ((double)points[i * row + (size_t)d] - k->h->lower[(size_t)d]) * (kLog2eHalfSqrt / k->bw[d]);
      pts[(size_t)d * pitch + j] = (float)c;
    }
  }
  codes.resize(pitch, -1);
  int nsplit = 1;
  unsigned tps = 1;
  choose_split(pitch, k->npad / SXMC_KDE_TILE, k->cus, nsplit, tps);
  if (sorted) sxkde::cutoff_split(pitch / 256, k->npad / SXMC_KDE_TILE, (unsigned long long)k->cus * 8, tps, nsplit);
  k->has_points = false;   // (until the new ones are in place: a failure below leaves an evaluator without points)
  if (pitch > k->d_codes.capacity()) {   // (the two grow together, both freed first; d_codes, allocated last, says whether both are there)
    SX_BUF(k->d_pts.reset());
    SX_BUF(k->d_codes.reset());
    SX_BUF(k->d_pts.alloc(pitch * (size_t)D));
    SX_BUF(k->d_codes.alloc(pitch));
  }
  SX_BUF(k->d_part.grow((size_t)nsplit * pitch));
  SX_HIP(hipMemcpy(k->d_pts.get(), pts.data(), sizeof(float) * pts.size(), hipMemcpyHostToDevice));
  SX_HIP(hipMemcpy(k->d_codes.get(), codes.data(), sizeof(int) * pitch, hipMemcpyHostToDevice));
  k->live_waves = 0;
  if (sorted) {
    const size_t nwaves = pitch / sxkde::kCutWave;
    std::vector<unsigned> place(pitch, 0u);
    for (size_t j = 0; j < n; j++) place[j] = order[j];
    std::vector<unsigned char> live(pitch, 0);
    for (size_t j = 0; j < nlive; j++) live[j] = 1;   // (the live points stand first)
    std::vector<float> box(nwaves * (size_t)sxkde::kCutWaveBox);
    for (size_t w = 0; w < nwaves; w++) {
      sxkde::cutoff_wave_box(D, pts.data(), pitch, w * sxkde::kCutWave, sxkde::kCutWave, live.data(),
                             &box[w * sxkde::kCutWaveBox]);
      if (w * sxkde::kCutWave < nlive) k->live_waves++;
    }
    SX_BUF(k->d_inv.grow(pitch));
    SX_BUF(k->d_wave_box.grow(box.size()));
    SX_HIP(hipMemcpy(k->d_inv.get(), place.data(), sizeof(unsigned) * pitch, hipMemcpyHostToDevice));
    SX_HIP(hipMemcpy(k->d_wave_box.get(), box.data(), sizeof(float) * box.size(), hipMemcpyHostToDevice));
  }
  k->points_sorted = sorted;
  k->npoints = n;
  k->pitch = pitch;
  k->nsplit = nsplit;
  k->tiles_per_split = tps;
  k->has_points = true;
  return SXMC_OK;
}

// The factors of an adaptive evaluator that has its table, bandwidths and npad: the pilot on the device (kde_pilot),
// then g and lambda on the host in f64 (kde_adaptive.h) and the upload of d_lambda.  rows: the untransformed table on
// the host; inside: its in-domain rows in table order.
int set_local_factors(sxmc_kde* k, const float* rows, int nfields, const std::vector<size_t>& inside) {
  const int D = k->D;
  const size_t n = inside.size(), pitch = k->npad;
  SxKdePilotArgs a;
  std::memset(&a, 0, sizeof a);
  a.D = D;
  a.pitch = pitch;
  a.n = n;
  sxkde::pilot_split(n, a.per_split, a.nsplit);
  for (int d = 0; d < D; d++) a.h[d] = k->bw[d];
  a.prefactor = k->prefactor;
  std::vector<double> x((size_t)D * pitch, 0.0), s0(n * (size_t)(D + 1));
  for (size_t i = 0; i < k->nsamples; i++) {
    for (int d = 0; d < D; d++) x[(size_t)d * pitch + i] = (double)rows[i * (size_t)nfields + (size_t)d];
  }
  for (size_t j = 0; j < n; j++) {
    double mass = 1.0;
    for (int d = 0; d < D; d++) {
      const double v = (double)rows[inside[j] * (size_t)nfields + (size_t)d];
      const double r = 1.0 / (k->bw[d] * M_SQRT2);
      // (as the prepass writes it)
      mass = mass * (0.5 * (std::erfc((v - k->h->upper[(size_t)d]) * r) - std::erfc((v - k->h->lower[(size_t)d]) * r)));
      s0[j * (size_t)(D + 1) + (size_t)d] = v;
    }
    s0[j * (size_t)(D + 1) + (size_t)D] = 1.0 / mass;
  }
  DeviceBuffer<double> dx, ds, dpart, df;   // (device memory of this call, freed when it returns)
  SX_BUF(dx.alloc(x.size()));
  SX_BUF(ds.alloc(s0.size()));
  SX_BUF(dpart.alloc((size_t)a.nsplit * pitch));
  SX_BUF(df.alloc(pitch));
  const hipStream_t s = k->h->stream;
  SX_HIP(hipMemcpyAsync(dx.get(), x.data(), sizeof(double) * x.size(), hipMemcpyHostToDevice, s));
  SX_HIP(hipMemcpyAsync(ds.get(), s0.data(), sizeof(double) * s0.size(), hipMemcpyHostToDevice, s));
  SX_HIP(sx_kde_pilot(a, dx.get(), ds.get(), dpart.get(), df.get(), s));
  std::vector<double> f(pitch);
  SX_HIP(hipMemcpyAsync(f.data(), df.get(), sizeof(double) * pitch, hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  const double g = sxkde::pilot_scale(f.data(), inside);
  std::vector<double> lam(pitch, 1.0);
  for (size_t i = 0; i < k->nsamples; i++) lam[i] = sxkde::local_factor(f[i], g, k->sensitivity);
  SX_BUF(k->d_lambda.alloc(pitch));
  SX_HIP(hipMemcpy(k->d_lambda.get(), lam.data(), sizeof(double) * pitch, hipMemcpyHostToDevice));
  lam.resize(k->nsamples);
  k->lambda.swap(lam);
  return SXMC_OK;
}

// sxmc_kde_create (sensitivity 0: nothing adaptive is allocated or run) and sxmc_kde_create_adaptive
int kde_create(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields, int nobservables,
               const double* lower, size_t n_lower, const double* upper, size_t n_upper, const double* bandwidth_scale,
               size_t n_bandwidth_scale, unsigned dataset, double sensitivity, sxmc_kde_t* out) {
  // Eval::Eval validation, pdfz.cpp:64-82 (same order, same messages, as sxmc_hist_create)
  SX_REQUIRE(nfields > 0 && nsamples_floats % (size_t)nfields == 0,
             "Length of samples array is not divisible by number of fields.");
  SX_REQUIRE(nobservables != 0, "Number of observables in PDF is zero.");
  SX_REQUIRE(nobservables > 0 && nobservables <= nfields,
             "Number of observables cannot be greater than number of fields.");
  SX_REQUIRE((int)n_upper == nobservables, "Number of upper bounds must be same as number of observables.");
  SX_REQUIRE((int)n_lower == nobservables, "Number of lower bounds must be same as number of observables.");
  SX_REQUIRE((int)n_bandwidth_scale == nobservables, "Number of bandwidth scales must be same as number of observables.");
  SX_REQUIRE(nfields <= SXMC_MAX_NFIELDS,
             "Exceeded maximum number of fields per sample. Edit MAX_NFIELDS in pdfz.cpp to fix this!");
  SX_REQUIRE(nobservables <= SXMC_KDE_MAX_DIM, "EvalKernel supports at most 4 observables.");
  SX_REQUIRE(lower && upper && bandwidth_scale, "null argument");
  for (int d = 0; d < nobservables; d++) {
    SX_REQUIRE(std::isfinite(bandwidth_scale[d]) && bandwidth_scale[d] > 0,
               "Bandwidth scales must be positive and finite.");
  }
  for (int d = 0; d < nobservables; d++) {
    SX_REQUIRE(upper[d] > lower[d], "Upper bound must be greater than lower bound.");
  }
  SX_REQUIRE(nsamples_floats == 0 || samples, "null samples");

  // Scott's rule over the untransformed samples inside the domain, in f64 on the host (before anything is allocated on
  // the device: a table that cannot set its bandwidths is refused without a GPU)
  std::vector<float> copy;
  const float* rows = samples;
  if (samples_on_device && nsamples_floats) {
    copy.resize(nsamples_floats);
    SX_HIP(hipMemcpy(copy.data(), samples, sizeof(float) * nsamples_floats, hipMemcpyDeviceToHost));
    rows = copy.data();
  }
  const int D = nobservables;
  const size_t nrows = nsamples_floats / (size_t)nfields;
  std::vector<size_t> inside;
  for (size_t i = 0; i < nrows; i++) {
    bool in = true;
    for (int d = 0; d < D; d++) {
      const double x = rows[i * (size_t)nfields + (size_t)d];
      in = in && x >= lower[d] && x < upper[d];
    }
    if (in) inside.push_back(i);
  }
  const size_t n = inside.size();
  SX_REQUIRE(n >= 2, "EvalKernel needs at least 2 samples inside the domain to set its bandwidths.");
  double bw[SXMC_KDE_MAX_DIM] = {0}, sigmas[SXMC_KDE_MAX_DIM] = {0}, prod_h = 1.0;
  for (int d = 0; d < D; d++) {
    double mean = 0.0, ss = 0.0;
    for (size_t i : inside) mean += rows[i * (size_t)nfields + (size_t)d];
    mean /= (double)n;
    for (size_t i : inside) {
      const double dx = rows[i * (size_t)nfields + (size_t)d] - mean;
      ss += dx * dx;
    }
    const double sigma = std::sqrt(ss / (double)(n - 1));
    SX_REQUIRE(sigma > 0, "EvalKernel bandwidth is zero: observable " + std::to_string(d) +
                              " has no spread inside the domain.");
    bw[d] = bandwidth_scale[d] * sigma * std::pow((double)n, -1.0 / (D + 4));
    sigmas[d] = sigma;
    prod_h *= bw[d];
  }

  const std::vector<int> nbins((size_t)nobservables, 1);
  sxmc_hist_t h = nullptr;
  int rc = sxmc_hist_create(samples, nsamples_floats, samples_on_device, nfields, nobservables, lower, n_lower, upper,
                            n_upper, nbins.data(), nbins.size(), dataset, &h);
  if (rc) return rc;
  std::unique_ptr<sxmc_kde> k(new sxmc_kde);
  k->h = h;
  k->D = D;
  k->nsamples = h->nsamples;
  for (int d = 0; d < D; d++) {
    k->bw[d] = bw[d];
    k->sigma[d] = sigmas[d];
    k->scale[d] = bandwidth_scale[d];
  }
  k->n_inside = n;
  k->prefactor = 1.0 / (std::pow(2.0 * M_PI, 0.5 * D) * prod_h);
  k->npad = std::max<size_t>(SXMC_KDE_TILE, (k->nsamples + SXMC_KDE_TILE - 1) / SXMC_KDE_TILE * SXMC_KDE_TILE);
  if (sensitivity > 0) {
    k->sensitivity = sensitivity;
    rc = set_local_factors(k.get(), rows, nfields, inside);
    if (rc) return rc;
  }
  rc = cleared_rows(k.get());
  if (rc) return rc;
  DeviceProps props;
  if (get_props(props) == SXMC_OK && props.cus > 0) k->cus = props.cus;
  *out = k.release();
  return SXMC_OK;
}

}  // namespace

extern "C" {

int sxmc_kde_create(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields, int nobservables,
                    const double* lower, size_t n_lower, const double* upper, size_t n_upper,
                    const double* bandwidth_scale, size_t n_bandwidth_scale, unsigned dataset, sxmc_kde_t* out) {
  SX_REQUIRE(out, "null argument");
  *out = nullptr;
  return kde_create(samples, nsamples_floats, samples_on_device, nfields, nobservables, lower, n_lower, upper, n_upper,
                    bandwidth_scale, n_bandwidth_scale, dataset, 0.0, out);
}

int sxmc_kde_create_adaptive(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields,
                             int nobservables, const double* lower, size_t n_lower, const double* upper,
                             size_t n_upper, const double* bandwidth_scale, size_t n_bandwidth_scale, unsigned dataset,
                             double sensitivity, sxmc_kde_t* out) {
  SX_REQUIRE(out, "null argument");
  *out = nullptr;
  SX_REQUIRE(sxkde::valid_sensitivity(sensitivity), "Bandwidth sensitivity must be a number in [0, 1].");
  return kde_create(samples, nsamples_floats, samples_on_device, nfields, nobservables, lower, n_lower, upper, n_upper,
                    bandwidth_scale, n_bandwidth_scale, dataset, sensitivity, out);
}

int sxmc_kde_create_shared(sxmc_kde_t base, sxmc_kde_t* out) {
  SX_REQUIRE(base && out, "null argument");
  *out = nullptr;
  sxmc_hist_t h = nullptr;
  int rc = sxmc_hist_create_shared(base->h, &h);   // the table (reference counted), the systematics, a stream
  if (rc) return rc;
  std::unique_ptr<sxmc_kde> k(new sxmc_kde);
  k->h = h;
  k->D = base->D;
  k->nsamples = base->nsamples;
  k->npad = base->npad;
  for (int d = 0; d < SXMC_KDE_MAX_DIM; d++) {
    k->bw[d] = base->bw[d];
    k->sigma[d] = base->sigma[d];
    k->scale[d] = base->scale[d];
  }
  k->n_inside = base->n_inside;
  k->prefactor = base->prefactor;
  k->cus = base->cus;
  if (base->d_lambda) {   // the factors are copied, never recomputed
    k->sensitivity = base->sensitivity;
    k->lambda = base->lambda;
    SX_BUF(k->d_lambda.alloc(k->npad));
    SX_HIP(hipMemcpy(k->d_lambda.get(), base->d_lambda.get(), sizeof(double) * k->npad, hipMemcpyDeviceToDevice));
  }
  rc = cleared_rows(k.get());
  if (rc) return rc;
  if (base->cutoff > 0) {   // the base's R on the base's order
    k->d_perm = base->d_perm;
    rc = cutoff_buffers(k.get());
    if (rc) return rc;
    k->cutoff = base->cutoff;
    k->qcut = base->qcut;
  }
  *out = k.release();
  return SXMC_OK;
}

int sxmc_kde_destroy(sxmc_kde_t k) {
  if (!k) return SXMC_OK;
  (void)order_after_caller(k);
  if (k->h && k->h->stream) (void)hipStreamSynchronize(k->h->stream);
  delete k;   // (the table's evaluator, then the buffers)
  return SXMC_OK;
}

int sxmc_kde_add_systematic(sxmc_kde_t k, int type, int obs, int extra_field, int npars, const short* pars) {
  SX_REQUIRE(k, "null evaluator");
  int rc = sxmc_hist_add_systematic(k->h, type, obs, extra_field, npars, pars);
  if (rc) return rc;
  // the prepass runs the fill's run-time decoded program: up to 7 columns, one coefficient per lane
  std::vector<int> slots;
  member_slots(k->h, slots);
  int ncoef = 0;
  for (const HostSyst& s : k->h->systs) ncoef += (int)s.pars.size();
  if (slots.size() > 7 || ncoef > 64) {
    k->h->systs.pop_back();
    return fail(SXMC_ERR_INVALID, "EvalKernel: the systematics read more than 7 fields or have more than 64 "
                                  "coefficients in all");
  }
  return SXMC_OK;
}

int sxmc_kde_set_eval_points(sxmc_kde_t k, const float* points, size_t npoints_floats) {
  SX_REQUIRE(k, "null evaluator");
  const int D = k->D;
  const size_t row = (size_t)D + 1;
  SX_REQUIRE(npoints_floats % row == 0,
             "Number of entries in evaluation points array not divisible by number of observables.");
  SX_REQUIRE(npoints_floats == 0 || points, "null points");
  const size_t n = npoints_floats / row;
  SX_REQUIRE(n <= (size_t)INT_MAX, "too many evaluation points");
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));   // (an evaluation in flight reads the arrays replaced here)
  k->has_points = false;
  k->host_points.assign(points, points + npoints_floats);
  return plan_points(k);
}

int sxmc_kde_set_pdf_value_buffer(sxmc_kde_t k, float* d_output, int offset, int stride) {
  SX_REQUIRE(k, "null evaluator");
  k->pdf = d_output;
  k->pdf_off = offset;
  k->pdf_stride = stride;
  return SXMC_OK;
}
int sxmc_kde_set_normalization_buffer(sxmc_kde_t k, unsigned* d_norm, int offset) {
  SX_REQUIRE(k, "null evaluator");
  k->norm = d_norm;
  k->norm_off = offset;
  return SXMC_OK;
}
int sxmc_kde_set_parameter_buffer(sxmc_kde_t k, const double* d_params, int offset, int stride) {
  SX_REQUIRE(k, "null evaluator");
  k->params = d_params;
  k->par_off = offset;
  k->par_stride = stride;
  return SXMC_OK;
}

}  // extern "C"

namespace {

// An evaluation's launches on stream s: norm clear, prepass, and for a lookup the pair sum and the combine.  No
// allocation, no blocking copy, no wait: what a recording tolerates.
int kde_launch(sxmc_kde* k, int do_eval_pdf, hipStream_t s) {
  if (!k->norm) return fail(SXMC_ERR_STATE, "evaluation before SetNormalizationBuffer");
  if (!k->h->systs.empty() && !k->params) return fail(SXMC_ERR_STATE, "evaluation before SetParameterBuffer");
  const bool lookup = do_eval_pdf && k->has_points && k->npoints > 0;
  if (lookup && !k->pdf) return fail(SXMC_ERR_STATE, "evaluation before SetPDFValueBuffer");
  SxSignalDesc d;
  fill_desc(k->h, d);
  d.params = k->params ? k->params + k->par_off : nullptr;
  d.param_stride = k->par_stride;
  SxKdeArgs a;
  std::memset(&a, 0, sizeof a);
  a.rows = k->d_rows.get();
  a.npad = k->npad;
  a.norm = k->norm + k->norm_off;
  for (int i = 0; i < k->D; i++) {
    a.lower[i] = k->h->lower[(size_t)i];
    a.upper[i] = k->h->upper[(size_t)i];
    a.cscale[i] = kLog2eHalfSqrt / k->bw[i];
    a.inv_h_sqrt2[i] = 1.0 / (k->bw[i] * M_SQRT2);
  }
  a.lambda = k->d_lambda.get();
  SX_HIP(hipMemsetAsync(a.norm, 0, sizeof(unsigned), s));
  SX_HIP(sx_kde_prepass(d, a, s));
  if (lookup) {
    const unsigned ntiles = (unsigned)(k->npad / SXMC_KDE_TILE);
    if (k->cutoff > 0) {
      if (!k->points_sorted || !k->d_perm) return fail(SXMC_ERR_STATE, "EvalKernel: the cutoff's point plan is missing");
      const bool adaptive = k->d_lambda.get() != nullptr;
      SX_HIP(hipMemsetAsync(k->d_visited.get(), 0, sizeof(unsigned long long) * kVisitedWords, s));
      SX_HIP(sx_kde_cutoff_gather(k->D, adaptive, k->d_rows.get(), k->d_perm->get(), ntiles, k->d_sorted.get(),
                                  k->d_tile_box.get(), s));
      SX_HIP(sx_kde_pairs_cutoff(k->D, adaptive, k->d_pts.get(), k->pitch, k->d_sorted.get(), k->d_tile_box.get(),
                                 k->d_wave_box.get(), k->tiles_per_split, ntiles, k->nsplit, k->qcut, k->d_part.get(),
                                 k->d_visited.get(), s));
      SX_HIP(sx_kde_combine_sorted(k->d_part.get(), k->pitch, k->nsplit, k->npoints, k->d_codes.get(), k->d_inv.get(),
                                   a.norm, k->prefactor, k->pdf + k->pdf_off, (long)k->pdf_stride, s));
    } else if (k->d_lambda.get()) {
      SX_HIP(sx_kde_pairs_adaptive(k->D, k->d_pts.get(), k->pitch, k->d_rows.get(), k->tiles_per_split, ntiles, k->nsplit,
                                   k->d_part.get(), s));
    } else {
      SX_HIP(sx_kde_pairs(k->D, k->d_pts.get(), k->pitch, k->d_rows.get(), k->tiles_per_split, ntiles, k->nsplit, k->d_part.get(), s));
    }
    if (!(k->cutoff > 0)) {
      SX_HIP(sx_kde_combine(k->d_part.get(), k->pitch, k->nsplit, k->npoints, k->d_codes.get(), a.norm, k->prefactor,
                            k->pdf + k->pdf_off, (long)k->pdf_stride, s));
    }
  }
  k->last_cut = lookup && k->cutoff > 0;
  k->last_possible = k->last_cut ? (unsigned long long)k->live_waves * (k->npad / SXMC_KDE_TILE) : 0ull;
  k->evaluated = true;
  k->evaluations++;
  return SXMC_OK;
}

}  // namespace

extern "C" {

int sxmc_kde_eval_async(sxmc_kde_t k, int do_eval_pdf) {
  SX_REQUIRE(k, "null evaluator");
  int rc = order_after_caller(k);
  if (rc) return rc;
  k->own_pending = true;
  return kde_launch(k, do_eval_pdf, k->h->stream);
}

int sxmc_kde_eval_on_stream_async(sxmc_kde_t k, int do_eval_pdf, sxmc_stream_t s) {
  SX_REQUIRE(k, "null evaluator");
  const hipStream_t st = (hipStream_t)s;
  if (k->own_pending && st != k->h->stream) {
    // (work on the evaluator's own stream that nothing has waited for: it reads and writes what this launch does)
    if (t_capturing) return fail(SXMC_ERR_STATE, "EvalKernel: EvalFinished before recording evaluations on another stream");
    SX_HIP(hipStreamSynchronize(k->h->stream));
    k->own_pending = false;
  }
  if (k->ext_pending && k->ext_stream != st) {
    int rc = order_after_caller(k);
    if (rc) return rc;
  }
  int rc = kde_launch(k, do_eval_pdf, st);
  if (rc) return rc;
  if (st != k->h->stream) {
    k->ext_stream = st;
    k->ext_pending = true;
  } else {
    k->own_pending = true;
  }
  return SXMC_OK;
}

int sxmc_kde_eval_finished(sxmc_kde_t k) {
  SX_REQUIRE(k, "null evaluator");
  int rc = order_after_caller(k);
  if (rc) return rc;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  k->own_pending = false;
  return SXMC_OK;
}

int sxmc_kde_parameters_read(sxmc_kde_t k, short* pars, size_t cap, size_t* n) {
  SX_REQUIRE(k && n && (pars || cap == 0), "null argument");
  size_t count = 0;
  for (const HostSyst& s : k->h->systs) {
    for (short p : s.pars) {
      if (count < cap) pars[count] = p;
      count++;
    }
  }
  *n = count;
  return SXMC_OK;
}

int sxmc_kde_evaluation_count(sxmc_kde_t k, unsigned long long* n) {
  SX_REQUIRE(k && n, "null argument");
  *n = k->evaluations;
  return SXMC_OK;
}

int sxmc_kde_get_stream(sxmc_kde_t k, sxmc_stream_t* s) {
  SX_REQUIRE(k && s, "null argument");
  *s = k->h->stream;
  return SXMC_OK;
}
int sxmc_kde_bandwidths(sxmc_kde_t k, double* h, size_t n) {
  SX_REQUIRE(k && h, "null argument");
  SX_REQUIRE(n == (size_t)k->D, "bandwidth buffer size mismatch");
  for (int d = 0; d < k->D; d++) h[d] = k->bw[d];
  return SXMC_OK;
}
int sxmc_kde_sensitivity(sxmc_kde_t k, double* v) {
  SX_REQUIRE(k && v, "null argument");
  *v = k->sensitivity;
  return SXMC_OK;
}
int sxmc_kde_local_factors(sxmc_kde_t k, double* lambda, size_t n) {
  SX_REQUIRE(k && (lambda || n == 0), "null argument");
  SX_REQUIRE(n == k->nsamples, "local factor buffer size mismatch");
  for (size_t i = 0; i < n; i++) lambda[i] = k->d_lambda ? k->lambda[i] : 1.0;
  return SXMC_OK;
}
int sxmc_kde_nsamples(sxmc_kde_t k, size_t* v) {
  SX_REQUIRE(k && v, "null argument");
  *v = k->nsamples;
  return SXMC_OK;
}
int sxmc_kde_set_cutoff(sxmc_kde_t k, double R) {
  SX_REQUIRE(sxkde::valid_cutoff(R), "Bandwidth cutoff must be 0 or a number >= 1 (infinity allowed).");
  SX_REQUIRE(k, "null evaluator");
  if (t_capturing) return fail(SXMC_ERR_STATE, "EvalKernel: not while recording a graph");
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  k->own_pending = false;
  if (R > 0) {
    if (!k->d_perm) {
      if (int rc_ = cutoff_sample_order(k)) return rc_;
    }
    if (int rc_ = cutoff_buffers(k)) return rc_;
  }
  const bool replan = k->has_points && (R > 0) != k->points_sorted;
  k->cutoff = R;
  k->qcut = sxkde::cutoff_qcut(R);
  if (replan) return plan_points(k);
  return SXMC_OK;
}
int sxmc_kde_cutoff(sxmc_kde_t k, double* R) {
  SX_REQUIRE(k && R, "null argument");
  *R = k->cutoff;
  return SXMC_OK;
}
int sxmc_kde_cutoff_stats(sxmc_kde_t k, unsigned long long* tiles_visited, unsigned long long* tiles_possible) {
  SX_REQUIRE(k && tiles_visited && tiles_possible, "null argument");
  *tiles_visited = 0;
  *tiles_possible = 0;
  if (!k->evaluated || !k->last_cut) return SXMC_OK;
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  std::vector<unsigned long long> counters(kVisitedWords);
  SX_HIP(hipMemcpy(counters.data(), k->d_visited.get(), sizeof(unsigned long long) * kVisitedWords, hipMemcpyDeviceToHost));
  for (int c = 0; c < sxkde::kCutCounters; c++) *tiles_visited += counters[(size_t)c * sxkde::kCutCounterStride];
  *tiles_possible = k->last_possible;
  return SXMC_OK;
}
int sxmc_kde_cutoff_boxes(sxmc_kde_t k, float* tile_boxes, size_t ntile_floats, float* wave_boxes, size_t nwave_floats) {
  SX_REQUIRE(k && tile_boxes && wave_boxes, "null argument");
  if (!(k->cutoff > 0) || !k->has_points || !k->points_sorted) {
    return fail(SXMC_ERR_STATE, "EvalKernel: no boxes without a cutoff and evaluation points");
  }
  SX_REQUIRE(ntile_floats == k->npad / SXMC_KDE_TILE * (size_t)sxkde::kCutBox &&
                 nwave_floats == k->pitch / sxkde::kCutWave * (size_t)sxkde::kCutWaveBox,
             "cutoff box buffer size mismatch");
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  SX_HIP(hipMemcpy(tile_boxes, k->d_tile_box.get(), sizeof(float) * ntile_floats, hipMemcpyDeviceToHost));
  SX_HIP(hipMemcpy(wave_boxes, k->d_wave_box.get(), sizeof(float) * nwave_floats, hipMemcpyDeviceToHost));
  return SXMC_OK;
}
int sxmc_kde_npoints(sxmc_kde_t k, size_t* v) {
  SX_REQUIRE(k && v, "null argument");
  *v = k->has_points ? k->npoints : 0;
  return SXMC_OK;
}

}  // extern "C"

namespace {

// Lists the in-domain rows of the last evaluation on the evaluator's stream and returns their count n (= the norm of
// that evaluation): after it, d_flag + 2 npad holds their row numbers in table order.
int kde_compact(sxmc_kde_t k, unsigned& n) {
  if (!k->evaluated) {
    return fail(SXMC_ERR_STATE, "EvalKernel: nothing to draw from before an evaluation (EvalAsync first)");
  }
  SX_REQUIRE(k->npad <= 0x7FFFFFFFull, "EvalKernel: too many samples to draw from");
  if (int rc_ = order_after_caller(k)) return rc_;
  const hipStream_t s = k->h->stream;
  if (!k->d_flag.get()) {
    SX_HIP(hipStreamSynchronize(s));   // (allocation next to queued work: settle it first)
    if (!k->d_scan_temp.get()) {
      size_t temp = 0;
      SX_HIP(sx_inclusive_sum_u32(nullptr, nullptr, (int)k->npad, nullptr, temp, s));
      SX_BUF(k->d_scan_temp.alloc(std::max<size_t>(temp, 16)));
      k->scan_temp_bytes = temp;
    }
    SX_BUF(k->d_flag.alloc(3 * k->npad));
  }
  unsigned* flag = k->d_flag.get();
  unsigned* pos = flag + k->npad;
  unsigned* idx = pos + k->npad;
  SX_HIP(sx_kde_compact(k->d_rows.get(), k->rowlen(), k->npad, flag, pos, idx, k->d_scan_temp.get(), k->scan_temp_bytes, s));
  SX_HIP(hipMemcpyAsync(&n, pos + (k->npad - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  return SXMC_OK;
}

}  // namespace

extern "C" {

int sxmc_kde_sample_pool(sxmc_kde_t k, size_t* n) {
  SX_REQUIRE(k && n, "null argument");
  unsigned c = 0;
  const int rc = kde_compact(k, c);
  if (rc) return rc;
  *n = c;
  return SXMC_OK;
}

int sxmc_kde_random_sample(sxmc_kde_t k, size_t nobserved, unsigned long long seed, const float* lowers,
                           const float* uppers, float* h_events) {
  SX_REQUIRE(k && (h_events || nobserved == 0), "null argument");
  SX_REQUIRE((lowers == nullptr) == (uppers == nullptr), "give both cut arrays or neither");
  if (!k->evaluated) {
    return fail(SXMC_ERR_STATE, "EvalKernel: nothing to draw from before an evaluation (EvalAsync first)");
  }
  if (nobserved == 0) return SXMC_OK;
  unsigned n = 0;
  int rc = kde_compact(k, n);
  if (rc) return rc;
  if (n == 0) {
    return fail(SXMC_ERR_STATE, "EvalKernel: the last evaluation left no sample inside the domain: nothing to draw from");
  }
  const int D = k->D;
  SxKdeSampleArgs g;
  std::memset(&g, 0, sizeof g);
  for (int d = 0; d < D; d++) {
    const double lo = k->h->lower[(size_t)d], hi = k->h->upper[(size_t)d];
    g.lower[d] = lo;
    g.upper[d] = hi;
    g.h[d] = k->bw[d];
    g.inv_cscale[d] = k->bw[d] / kLog2eHalfSqrt;
    float b = (float)lo, t = (float)hi;
    if ((double)b < lo) b = std::nextafter(b, std::numeric_limits<float>::infinity());
    while (!((double)t < hi)) t = std::nextafter(t, -std::numeric_limits<float>::infinity());
    g.bottom[d] = b;
    g.top[d] = t;
    g.cut_lo[d] = lowers ? lowers[d] : 0.0f;
    g.cut_hi[d] = uppers ? uppers[d] : 0.0f;
  }
  g.has_cuts = lowers ? 1 : 0;
  g.dataset = (float)k->h->dataset;
  const size_t row = (size_t)D + 1;
  float* d_out = nullptr;
  unsigned* d_exhausted = nullptr;
  rc = sample_buffer(k->h, nobserved, row, d_out, d_exhausted);   // (the histogram evaluator's, on the same stream)
  if (rc) return rc;
  const unsigned* idx = k->d_flag.get() + 2 * k->npad;
  SX_HIP(sx_kde_sample(D, k->d_rows.get(), k->d_lambda.get(), idx, n, g, seed, nobserved, d_out, d_exhausted, k->h->stream));
  return sample_read_back(k->h, nobserved, row, ": the cuts leave (almost) none of the kernel-density PDF's mass",
                          h_events);
}

int sxmc_kde_project(sxmc_kde_t k, int obs, int nbins, double* h_prob) {
  SX_REQUIRE(k && h_prob, "null argument");
  SX_REQUIRE(obs >= 0 && obs < k->D, "EvalKernel: no such observable to project onto");
  SX_REQUIRE(nbins >= 1, "EvalKernel: a projection needs at least one bin");
  if (!k->evaluated) {
    return fail(SXMC_ERR_STATE, "EvalKernel: nothing to project before an evaluation (EvalAsync first)");
  }
  SxKdeProjectArgs a;
  std::memset(&a, 0, sizeof a);
  a.D = k->D;
  a.obs = obs;
  a.nbins = nbins;
  a.npad = k->npad;
  // the sample rows are cut the same way on every device: at most 1024 splits of whole tiles
  const unsigned long long tile = SXMC_KDE_TILE;
  a.rows_per_split = (unsigned)(((k->npad + 1023) / 1024 + tile - 1) / tile * tile);
  a.nsplit = (unsigned)((k->npad + a.rows_per_split - 1) / a.rows_per_split);
  a.pitch = ((unsigned long long)nbins + SXMC_KDE_PROJ_LANES - 1) / SXMC_KDE_PROJ_LANES * SXMC_KDE_PROJ_LANES;
  a.lower = k->h->lower[(size_t)obs];
  a.upper = k->h->upper[(size_t)obs];
  a.h = k->bw[obs];
  a.cunit = kLog2eHalfSqrt;
  a.lambda = k->d_lambda.get();
  if (int rc_ = order_after_caller(k)) return rc_;
  const hipStream_t s = k->h->stream;
  // [2 npad] per-row scratch ([3 npad] when adaptive), [nsplit][pitch] partials, [nbins] result, the count
  const size_t off_prob = (k->d_lambda ? 3 : 2) * k->npad + (size_t)a.nsplit * a.pitch;
  const size_t need = off_prob + (size_t)nbins + 1;
  if (need > k->d_proj.capacity()) {
    SX_HIP(hipStreamSynchronize(s));   // (allocation next to queued work: settle it first)
    SX_BUF(k->d_proj.grow(need));
  }
  double* d_prob = k->d_proj.get() + off_prob;
  unsigned* d_count = reinterpret_cast<unsigned*>(d_prob + nbins);
  SX_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
  SX_HIP(sx_kde_project(k->d_rows.get(), a, k->d_proj.get(), d_count, d_prob, s));
  SX_HIP(hipMemcpyAsync(h_prob, d_prob, sizeof(double) * (size_t)nbins, hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  return SXMC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------ cross-validation (kde_cv.h)
namespace {

// One search's rows on the device: the scored subset of the untransformed in-domain rows, read back from the table.
struct CvRows {
  int D = 0;
  size_t m = 0, pitch = 0;
  DeviceBuffer<double> d_x;     // [D][pitch]
  std::vector<double> rows;     // [m][D], table order
};

// The subset kde_cv.h names, of the f64 values of the float table at zero systematics.
int cv_rows(sxmc_kde* k, size_t max_rows, CvRows& r) {
  const int D = k->D;
  const size_t n = k->nsamples;
  if (int rc_ = order_after_caller(k)) return rc_;
  std::vector<float> cols((size_t)D * n);
  for (int d = 0; d < D; d++) {   // (column d of the column-major table is observable d)
    SX_HIP(hipMemcpy(cols.data() + (size_t)d * n, k->h->store->d_cols.get() + (size_t)d * k->h->pitch, sizeof(float) * n,
                     hipMemcpyDeviceToHost));
  }
  std::vector<size_t> inside;
  for (size_t i = 0; i < n; i++) {
    bool in = true;
    for (int d = 0; d < D; d++) {
      const double x = cols[(size_t)d * n + i];
      in = in && x >= k->h->lower[(size_t)d] && x < k->h->upper[(size_t)d];
    }
    if (in) inside.push_back(i);
  }
  const std::vector<size_t> pick = sxkde::cv_subset(inside.size(), max_rows);
  r.D = D;
  r.m = pick.size();
  SX_REQUIRE(r.m >= 2, "Cross-validation needs at least 2 rows to score.");
  SX_REQUIRE(r.m <= 0x7FFFFF00ull, "Cross-validation: too many rows to score (set max_rows).");
  r.pitch = (r.m + 255) / 256 * 256;
  r.rows.resize(r.m * (size_t)D);
  std::vector<double> x((size_t)D * r.pitch, 0.0);
  for (size_t j = 0; j < r.m; j++) {
    for (int d = 0; d < D; d++) {
      const double v = cols[(size_t)d * n + inside[pick[j]]];
      r.rows[j * (size_t)D + (size_t)d] = v;
      x[(size_t)d * r.pitch + j] = v;
    }
  }
  SX_BUF(r.d_x.alloc(x.size()));
  SX_HIP(hipMemcpy(r.d_x.get(), x.data(), sizeof(double) * x.size(), hipMemcpyHostToDevice));
  return SXMC_OK;
}

// score(h_c) of K candidates (bw[c * D + d], absolute) on the rows of r.
int cv_scan(sxmc_kde* k, const CvRows& r, const double* bw, int K, double* scores) {
  const int D = r.D;
  SxKdeCvArgs a;
  std::memset(&a, 0, sizeof a);
  a.D = D;
  a.K = K;
  a.KP = sx_kde_cv_padded(K);
  a.m = (unsigned)r.m;
  a.pitch = r.pitch;
  sxkde::cv_split(r.m, K, a.per_split, a.nsplit);
  for (int d = 0; d < D; d++) {
    a.lower[d] = k->h->lower[(size_t)d];
    a.upper[d] = k->h->upper[(size_t)d];
  }
  a.prefactor = 1.0 / (std::pow(2.0 * M_PI, 0.5 * D) * (double)(r.m - 1));
  const size_t KP = (size_t)a.KP, row = (size_t)D + KP;
  // the candidates' constants; the padding has g = 0 and weighs 0
  std::vector<double> cand(2 * KP * (size_t)D + KP, 0.0);
  for (size_t c = 0; c < KP; c++) {
    double prod_h = 1.0;
    for (int d = 0; d < D; d++) {
      const double h = c < (size_t)K ? bw[c * (size_t)D + (size_t)d] : 1.0;
      cand[c * (size_t)D + (size_t)d] = c < (size_t)K ? 1.0 / (2.0 * h * h) : 0.0;
      cand[KP * (size_t)D + c * (size_t)D + (size_t)d] = 1.0 / (h * M_SQRT2);
      prod_h *= h;
    }
    cand[2 * KP * (size_t)D + c] = prod_h;
  }
  std::vector<double> s0(r.m * row, 0.0);
  for (size_t j = 0; j < r.m; j++) {
    for (int d = 0; d < D; d++) s0[j * row + (size_t)d] = r.rows[j * (size_t)D + (size_t)d];
  }
  DeviceBuffer<double> ds, dc, dpart, dln;   // (device memory of this scan, freed when it returns)
  SX_BUF(ds.alloc(s0.size()));
  SX_BUF(dc.alloc(cand.size()));
  SX_BUF(dpart.alloc((size_t)a.nsplit * KP * r.pitch));
  SX_BUF(dln.alloc((size_t)K * r.pitch));
  const hipStream_t s = k->h->stream;
  SX_HIP(hipMemcpyAsync(ds.get(), s0.data(), sizeof(double) * s0.size(), hipMemcpyHostToDevice, s));
  SX_HIP(hipMemcpyAsync(dc.get(), cand.data(), sizeof(double) * cand.size(), hipMemcpyHostToDevice, s));
  SX_HIP(sx_kde_cv_scan(a, r.d_x.get(), ds.get(), dc.get(), dpart.get(), dln.get(), s));
  std::vector<double> lnf((size_t)K * r.pitch);
  SX_HIP(hipMemcpyAsync(lnf.data(), dln.get(), sizeof(double) * lnf.size(), hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < K; c++) {   // the m logarithms in table order
    double sum = 0.0;
    for (size_t i = 0; i < r.m; i++) sum += lnf[(size_t)c * r.pitch + i];
    scores[c] = sum / (double)r.m;
  }
  return SXMC_OK;
}

int cv_check_candidates(const sxmc_kde* k, const double* bw, int K) {
  SX_REQUIRE(K >= 1 && K <= sxkde::kCvMaxCandidates, "Cross-validation scores between 1 and 32 candidates at a time.");
  for (size_t i = 0; i < (size_t)K * (size_t)k->D; i++) {
    SX_REQUIRE(std::isfinite(bw[i]) && bw[i] > 0 && std::isfinite(1.0 / (2.0 * bw[i] * bw[i])) && 2.0 * bw[i] * bw[i] > 0,
               "Candidate bandwidths must be positive and finite.");
  }
  return SXMC_OK;
}

}  // namespace

extern "C" {

int sxmc_kde_bandwidth_scale(sxmc_kde_t k, double* scale, size_t n) {
  SX_REQUIRE(k && scale, "null argument");
  SX_REQUIRE(n == (size_t)k->D, "bandwidth scale buffer size mismatch");
  for (int d = 0; d < k->D; d++) scale[d] = k->scale[d];
  return SXMC_OK;
}

int sxmc_kde_cv_scores(sxmc_kde_t k, const double* bandwidths, int ncandidates, size_t max_rows, double* scores,
                       size_t* rows_used) {
  SX_REQUIRE(k && bandwidths && scores, "null argument");
  if (int rc_ = cv_check_candidates(k, bandwidths, ncandidates)) return rc_;
  SX_REQUIRE(sxkde::cv_subset_size(k->n_inside, max_rows) >= 2, "Cross-validation needs at least 2 rows to score.");
  CvRows r;
  int rc = cv_rows(k, max_rows, r);
  if (rc) return rc;
  if (rows_used) *rows_used = r.m;
  return cv_scan(k, r, bandwidths, ncandidates, scores);
}

int sxmc_kde_cv_select(sxmc_kde_t k, double lo, double hi, int steps, int per_observable, size_t max_rows,
                       double* scale_out, size_t n_scale, double* score, double* score_at_one, int* at_edge,
                       size_t* rows_used, int* nscans, double* scan_grid, double* scan_scores, int* scan_chosen) {
  SX_REQUIRE(k && scale_out, "null argument");
  SX_REQUIRE(n_scale == (size_t)k->D, "bandwidth scale buffer size mismatch");
  if (const char* why = sxkde::cv_grid_error(lo, hi, steps)) return fail(SXMC_ERR_INVALID, why);
  SX_REQUIRE(sxkde::cv_subset_size(k->n_inside, max_rows) >= 2, "Cross-validation needs at least 2 rows to score.");
  CvRows r;
  int rc = cv_rows(k, max_rows, r);
  if (rc) return rc;
  const int D = k->D;
  // the subset's candidates are scaled to its own size: h_cd = s_cd sigma_d m^(-1/(D+4)), sigma_d over all n rows
  const double shrink = std::pow((double)r.m, -1.0 / (D + 4));
  sxkde::CvOptions o;
  o.lo = lo;
  o.hi = hi;
  o.steps = steps;
  o.per_observable = per_observable != 0;
  o.max_rows = max_rows;
  sxkde::CvReport rep;
  std::string error;
  rc = sxkde::cv_search(o, D, [&](const double* mult, int K, double* out) {
    std::vector<double> bw((size_t)K * (size_t)D);
    for (int c = 0; c < K; c++) {
      for (int d = 0; d < D; d++) bw[(size_t)c * D + d] = mult[(size_t)c * D + d] * k->sigma[d] * shrink;
    }
    if (int rc_ = cv_check_candidates(k, bw.data(), K)) return rc_;
    return cv_scan(k, r, bw.data(), K, out);
  }, rep, error);
  if (rc == -1) return fail(SXMC_ERR_INVALID, error);
  if (rc) return rc;
  for (int d = 0; d < D; d++) {
    scale_out[d] = rep.scale[(size_t)d];
    if (at_edge) at_edge[d] = rep.at_edge[(size_t)d];
  }
  if (score) *score = rep.score;
  if (score_at_one) *score_at_one = rep.score_at_one;
  if (rows_used) *rows_used = r.m;
  if (nscans) *nscans = (int)rep.scans.size();
  for (size_t s = 0; s < rep.scans.size(); s++) {
    for (int c = 0; c < steps; c++) {
      if (scan_grid) scan_grid[s * (size_t)steps + (size_t)c] = rep.scans[s].grid[(size_t)c];
      if (scan_scores) scan_scores[s * (size_t)steps + (size_t)c] = rep.scans[s].scores[(size_t)c];
    }
    if (scan_chosen) scan_chosen[s] = rep.scans[s].chosen;
  }
  return SXMC_OK;
}

}  // extern "C"
