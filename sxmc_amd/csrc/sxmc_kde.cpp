// sxmc_kde.cpp -- the evaluator behind pdfz::EvalKernel (sxmc_kde_*): the kernel-density PDF.  The contract is written
// out in include/sxmc_hip.h and sxmc_amd/include/sxmc/pdfz.h; the kernels are in kde_kernels.hip.  This unit holds
// creation, the points, the bindings, the launch, the streams and the accessors; cross-validation is in sxmc_kde_cv.cpp,
// what reads the last evaluation's rows (sampling, projection) in sxmc_kde_draw.cpp, the state in sxmc_kde_state.h.
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
// Weighted Monte Carlo samples (sxmc_kde_create_weighted; the host arithmetic in kde_weights.h): the rows' multiplicities
// are given at creation, where the bandwidths and the pilot read them, and kept in d_mult, padded with 0 to npad and
// shared with the table; with them the prepass, the sampler and the projection take their weighted forms.  Without,
// d_mult is null and every launch is the one it was.
//
// A cutoff radius (sxmc_kde_set_cutoff; the pure parts in kde_cutoff.h): the spatial order of the table rows is made on
// the host when a cutoff is first set and kept on the device (shared evaluators hold the same buffer); the points are
// planned in the same order by set_eval_points, which keeps the caller's points so that a change of R can plan them
// again.  Everything an evaluation needs is allocated there: kde_launch allocates nothing.  At R = 0 the launches are
// the ones above and the points stay in the caller's order.
#include "sxmc_kde_state.h"

#include "kde_adaptive.h"
#include "kde_weights.h"

using namespace sxhost;

int sxhost::order_after_caller(sxmc_kde* k) {
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

int sxhost::table_columns(sxmc_kde* k, std::vector<float>& cols) {
  const size_t n = k->nsamples;
  cols.resize((size_t)k->D * n);
  for (int d = 0; d < k->D && n; d++) {   // (column d of the column-major table is observable d)
    SX_HIP(hipMemcpy(cols.data() + (size_t)d * n, k->h->store->d_cols.get() + (size_t)d * k->h->pitch, sizeof(float) * n,
                     hipMemcpyDeviceToHost));
  }
  return SXMC_OK;
}

namespace {

// The cleared sample rows of a new evaluator that has its table (k->h) and npad.
int cleared_rows(sxmc_kde* k) {
  const size_t n = k->npad * (size_t)k->rowlen();
  SX_BUF(k->d_rows.alloc(n));
  SX_HIP(hipMemset(k->d_rows.get(), 0, sizeof(float) * n));
  return SXMC_OK;
}

// What an evaluation with a cutoff writes besides the rows: allocated once, cleared.
int cutoff_buffers(sxmc_kde* k) {
  const size_t ntiles = k->npad / SXMC_KDE_TILE;
  if (!k->cut.d_sorted.get()) {
    const size_t n = k->npad * (size_t)k->rowlen();
    SX_BUF(k->cut.d_sorted.alloc(n));
    SX_HIP(hipMemset(k->cut.d_sorted.get(), 0, sizeof(float) * n));
  }
  if (!k->cut.d_tile_box.get()) {
    std::vector<float> box(ntiles * (size_t)sxkde::kCutBox, 1.0f);
    for (size_t t = 0; t < ntiles; t++) sxkde::cutoff_empty_box(&box[t * sxkde::kCutBox], &box[t * sxkde::kCutBox + sxkde::kCutMaxDim]);
    SX_BUF(k->cut.d_tile_box.alloc(box.size()));
    SX_HIP(hipMemcpy(k->cut.d_tile_box.get(), box.data(), sizeof(float) * box.size(), hipMemcpyHostToDevice));
  }
  if (!k->cut.d_visited.get()) {
    SX_BUF(k->cut.d_visited.alloc(kVisitedWords));
    SX_HIP(hipMemset(k->cut.d_visited.get(), 0, sizeof(unsigned long long) * kVisitedWords));
  }
  return SXMC_OK;
}

// The spatial order of the table rows (kde_cutoff.h), from the untransformed table read back, onto the device.
int cutoff_sample_order(sxmc_kde* k) {
  const int D = k->D;
  const size_t n = k->nsamples;
  SX_REQUIRE(k->npad <= 0xFFFFFFFFull, "EvalKernel: too many samples for a cutoff");
  std::vector<float> cols, x((size_t)D * n);
  if (int rc_ = table_columns(k, cols)) return rc_;
  for (size_t i = 0; i < n; i++) {
    for (int d = 0; d < D; d++) x[i * (size_t)D + (size_t)d] = cols[(size_t)d * n + i];
  }
  const std::vector<uint32_t> order = sxkde::cutoff_sample_order(D, x.data(), (size_t)D, n, k->npad, k->h->lower.data(),
                                                                 k->h->upper.data());
  auto perm = std::make_shared<DeviceBuffer<unsigned>>();
  SX_BUF(perm->alloc(k->npad));
  SX_HIP(hipMemcpy(perm->get(), order.data(), sizeof(unsigned) * k->npad, hipMemcpyHostToDevice));
  k->cut.d_perm = perm;
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
  const bool sorted = k->cut.on();
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
  sxkde::pair_split(pitch, k->npad / SXMC_KDE_TILE, k->cus, nsplit, tps);
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
  k->cut.live_waves = 0;
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
      if (w * sxkde::kCutWave < nlive) k->cut.live_waves++;
    }
    SX_BUF(k->cut.d_inv.grow(pitch));
    SX_BUF(k->cut.d_wave_box.grow(box.size()));
    SX_HIP(hipMemcpy(k->cut.d_inv.get(), place.data(), sizeof(unsigned) * pitch, hipMemcpyHostToDevice));
    SX_HIP(hipMemcpy(k->cut.d_wave_box.get(), box.data(), sizeof(float) * box.size(), hipMemcpyHostToDevice));
  }
  k->cut.points_sorted = sorted;
  k->npoints = n;
  k->pitch = pitch;
  k->nsplit = nsplit;
  k->tiles_per_split = tps;
  k->has_points = true;
  return SXMC_OK;
}

// The factors of an adaptive evaluator that has its table, bandwidths and npad: the pilot on the device (kde_pilot),
// then g and lambda on the host in f64 (kde_adaptive.h) and the upload of d_lambda.  rows: the untransformed table on
// the host; inside: its in-domain rows in table order.  m: the rows' multiplicities or null -- with them a row's pilot
// weight is m_j / mass_j, their in-domain total s1 divides in place of n, and g weighs ln f_i by m_i.  The law sums
// "over the in-domain rows": a row of multiplicity 0 stays in s0 at weight 0 and adds +0.0 (pairs wasted at
// construction, the split over workgroups -- from the in-domain count alone -- the same as without multiplicities).
int set_local_factors(sxmc_kde* k, const float* rows, int nfields, const std::vector<size_t>& inside, const unsigned* m,
                      double s1) {
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
      mass = mass * sxkde::truncation_mass(v, k->h->lower[(size_t)d], k->h->upper[(size_t)d], r);   // (as the prepass)
      s0[j * (size_t)(D + 1) + (size_t)d] = v;
    }
    s0[j * (size_t)(D + 1) + (size_t)D] = (m ? (double)m[inside[j]] : 1.0) / mass;
  }
  DeviceBuffer<double> dx, ds, dpart, df;   // (device memory of this call, freed when it returns)
  SX_BUF(dx.alloc(x.size()));
  SX_BUF(ds.alloc(s0.size()));
  SX_BUF(dpart.alloc((size_t)a.nsplit * pitch));
  SX_BUF(df.alloc(pitch));
  const hipStream_t s = k->h->stream;
  SX_HIP(hipMemcpyAsync(dx.get(), x.data(), sizeof(double) * x.size(), hipMemcpyHostToDevice, s));
  SX_HIP(hipMemcpyAsync(ds.get(), s0.data(), sizeof(double) * s0.size(), hipMemcpyHostToDevice, s));
  SX_HIP(sx_kde_pilot(a, dx.get(), ds.get(), m ? s1 : 0.0, dpart.get(), df.get(), s));
  std::vector<double> f(pitch);
  SX_HIP(hipMemcpyAsync(f.data(), df.get(), sizeof(double) * pitch, hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  const double g = m ? sxkde::weighted_pilot_scale(f.data(), inside, m, s1) : sxkde::pilot_scale(f.data(), inside);
  std::vector<double> lam(pitch, 1.0);
  for (size_t i = 0; i < k->nsamples; i++) lam[i] = sxkde::local_factor(f[i], g, k->sensitivity);
  SX_BUF(k->d_lambda.alloc(pitch));
  SX_HIP(hipMemcpy(k->d_lambda.get(), lam.data(), sizeof(double) * pitch, hipMemcpyHostToDevice));
  lam.resize(k->nsamples);
  k->lambda.swap(lam);
  return SXMC_OK;
}

// The arguments every creation and sxmc_kde_weighted_bandwidths check alike.  Eval::Eval validation, pdfz.cpp:64-82
// (same order, same messages, as sxmc_hist_create)
int kde_check_arguments(const float* samples, size_t nsamples_floats, int nfields, int nobservables, const double* lower,
                        size_t n_lower, const double* upper, size_t n_upper, const double* bandwidth_scale,
                        size_t n_bandwidth_scale) {
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
  return SXMC_OK;
}

// The multiplicities' count and total, checked without a device.
int kde_check_multiplicities(const unsigned* m, size_t nm, size_t nrows) {
  SX_REQUIRE(nm == nrows, "EvalKernel sample multiplicities: " + std::to_string(nm) + " given for " + std::to_string(nrows) +
                              " rows of the table (one word per row)");
  unsigned long long total = 0;
  for (size_t i = 0; i < nm; i++) total += m[i];   // (at most 2^32 rows of less than 2^32 each: no overflow of 64 bits)
  if (total > 0xFFFFFFFFull) {
    return fail(SXMC_ERR_INVALID, "EvalKernel sample multiplicities: their total " + std::to_string(total) +
                                      " exceeds 4294967295, what the unsigned normalisation holds");
  }
  return SXMC_OK;
}

// What weighted_bandwidths refused, by name.
int kde_bandwidth_refusal(const sxkde::WeightedBandwidths& wb, bool weighted) {
  switch (wb.status) {
    case sxkde::kWeightsTooFew:
      if (!weighted) return fail(SXMC_ERR_INVALID, "EvalKernel needs at least 2 samples inside the domain to set its bandwidths.");
      return fail(SXMC_ERR_INVALID, "EvalKernel needs at least 2 samples of multiplicity > 0 inside the domain to set its "
                                    "bandwidths.");
    case sxkde::kWeightsNoFreedom:
      return fail(SXMC_ERR_INVALID, "EvalKernel sample multiplicities leave no degree of freedom (sum m - sum m^2 / sum m is "
                                    "not positive): no bandwidth.");
    case sxkde::kWeightsNoSpread:
      return fail(SXMC_ERR_INVALID, "EvalKernel bandwidth is zero: observable " + std::to_string(wb.observable) +
                                        " has no spread inside the domain.");
    default: return SXMC_OK;
  }
}

// sxmc_kde_create (sensitivity 0: nothing adaptive is allocated or run), sxmc_kde_create_adaptive and
// sxmc_kde_create_weighted (m: one multiplicity per table row on the host, or null: none)
int kde_create(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields, int nobservables,
               const double* lower, size_t n_lower, const double* upper, size_t n_upper, const double* bandwidth_scale,
               size_t n_bandwidth_scale, unsigned dataset, double sensitivity, const unsigned* m, size_t nm,
               sxmc_kde_t* out) {
  if (int rc_ = kde_check_arguments(samples, nsamples_floats, nfields, nobservables, lower, n_lower, upper, n_upper,
                                    bandwidth_scale, n_bandwidth_scale)) {
    return rc_;
  }

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
  const std::vector<size_t> inside = sxkde::rows_inside(rows, (size_t)nfields, 1, nrows, D, lower, upper);
  const size_t n = inside.size();
  // (kde_weights.h: with multiplicities Kish's n_eff stands where n stood and the moments weigh every row by m; without,
  // the same function gives the unweighted rule's bytes)
  if (m) {
    if (int rc_ = kde_check_multiplicities(m, nm, nrows)) return rc_;
  }
  const sxkde::WeightedBandwidths wb = sxkde::weighted_bandwidths(rows, (size_t)nfields, inside, D, bandwidth_scale, m);
  if (int rc_ = kde_bandwidth_refusal(wb, m != nullptr)) return rc_;
  double bw[SXMC_KDE_MAX_DIM] = {0}, sigmas[SXMC_KDE_MAX_DIM] = {0}, prod_h = 1.0;
  for (int d = 0; d < D; d++) {
    bw[d] = wb.h[d];
    sigmas[d] = wb.sigma[d];
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
  k->n_eff = wb.n_eff;
  k->npad = std::max<size_t>(SXMC_KDE_TILE, (k->nsamples + SXMC_KDE_TILE - 1) / SXMC_KDE_TILE * SXMC_KDE_TILE);
  if (m) {   // the library's own copy, 0 in the padding up to npad
    auto column = std::make_shared<DeviceBuffer<unsigned>>();
    SX_BUF(column->alloc(k->npad));
    // (on the evaluator's own stream, which carries every later launch, and waited for: `m` is the caller's)
    const hipStream_t s = k->h->stream;
    SX_HIP(hipMemsetAsync(column->get(), 0, sizeof(unsigned) * k->npad, s));
    if (nm) SX_HIP(hipMemcpyAsync(column->get(), m, sizeof(unsigned) * nm, hipMemcpyHostToDevice, s));
    SX_HIP(hipStreamSynchronize(s));
    k->d_mult = std::move(column);
    k->mult = std::make_shared<const std::vector<unsigned>>(m, m + nm);
    k->mult_total = 0;
    for (size_t i = 0; i < nm; i++) k->mult_total += m[i];
  }
  if (sensitivity > 0) {
    k->sensitivity = sensitivity;
    rc = set_local_factors(k.get(), rows, nfields, inside, m, wb.s1);
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
                    bandwidth_scale, n_bandwidth_scale, dataset, 0.0, nullptr, 0, out);
}

int sxmc_kde_create_adaptive(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields,
                             int nobservables, const double* lower, size_t n_lower, const double* upper,
                             size_t n_upper, const double* bandwidth_scale, size_t n_bandwidth_scale, unsigned dataset,
                             double sensitivity, sxmc_kde_t* out) {
  SX_REQUIRE(out, "null argument");
  *out = nullptr;
  SX_REQUIRE(sxkde::valid_sensitivity(sensitivity), "Bandwidth sensitivity must be a number in [0, 1].");
  return kde_create(samples, nsamples_floats, samples_on_device, nfields, nobservables, lower, n_lower, upper, n_upper,
                    bandwidth_scale, n_bandwidth_scale, dataset, sensitivity, nullptr, 0, out);
}

int sxmc_kde_create_weighted(const float* samples, size_t nsamples_floats, int samples_on_device, int nfields,
                             int nobservables, const double* lower, size_t n_lower, const double* upper,
                             size_t n_upper, const double* bandwidth_scale, size_t n_bandwidth_scale, unsigned dataset,
                             double sensitivity, const unsigned* multiplicities, size_t nmultiplicities,
                             sxmc_kde_t* out) {
  SX_REQUIRE(out, "null argument");
  *out = nullptr;
  SX_REQUIRE(sxkde::valid_sensitivity(sensitivity), "Bandwidth sensitivity must be a number in [0, 1].");
  return kde_create(samples, nsamples_floats, samples_on_device, nfields, nobservables, lower, n_lower, upper, n_upper,
                    bandwidth_scale, n_bandwidth_scale, dataset, sensitivity, multiplicities, nmultiplicities, out);
}

int sxmc_kde_weighted_bandwidths(const float* samples, size_t nsamples_floats, int nfields, int nobservables,
                                 const double* lower, size_t n_lower, const double* upper, size_t n_upper,
                                 const double* bandwidth_scale, size_t n_bandwidth_scale,
                                 const unsigned* multiplicities, size_t nmultiplicities, double* h, double* sigma,
                                 double* mean, double* n_eff, double* s1, double* s2) {
  if (int rc_ = kde_check_arguments(samples, nsamples_floats, nfields, nobservables, lower, n_lower, upper, n_upper,
                                    bandwidth_scale, n_bandwidth_scale)) {
    return rc_;
  }
  const size_t nrows = nsamples_floats / (size_t)nfields;
  if (multiplicities) {
    if (int rc_ = kde_check_multiplicities(multiplicities, nmultiplicities, nrows)) return rc_;
  }
  const std::vector<size_t> inside = sxkde::rows_inside(samples, (size_t)nfields, 1, nrows, nobservables, lower, upper);
  const sxkde::WeightedBandwidths wb =
      sxkde::weighted_bandwidths(samples, (size_t)nfields, inside, nobservables, bandwidth_scale, multiplicities);
  if (s1) *s1 = wb.s1;
  if (s2) *s2 = wb.s2;
  if (int rc_ = kde_bandwidth_refusal(wb, multiplicities != nullptr)) return rc_;
  for (int d = 0; d < nobservables; d++) {
    if (h) h[d] = wb.h[d];
    if (sigma) sigma[d] = wb.sigma[d];
    if (mean) mean[d] = wb.mean[d];
  }
  if (n_eff) *n_eff = wb.n_eff;
  return SXMC_OK;
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
  k->d_mult = base->d_mult;   // (the rows' multiplicities belong to the table: shared with it)
  k->mult = base->mult;
  k->mult_total = base->mult_total;
  k->n_eff = base->n_eff;
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
  if (base->cut.on()) {   // the base's R on the base's order
    k->cut.d_perm = base->cut.d_perm;
    rc = cutoff_buffers(k.get());
    if (rc) return rc;
    k->cut.cutoff = base->cut.cutoff;
    k->cut.qcut = base->cut.qcut;
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
  SX_HIP(sx_kde_prepass(d, a, k->mult_ptr(), s));
  if (lookup) {
    const unsigned ntiles = (unsigned)(k->npad / SXMC_KDE_TILE);
    const bool adaptive = k->adaptive();
    KdeCutoff& c = k->cut;
    if (c.on()) {
      if (!c.points_sorted || !c.d_perm) return fail(SXMC_ERR_STATE, "EvalKernel: the cutoff's point plan is missing");
      SX_HIP(hipMemsetAsync(c.d_visited.get(), 0, sizeof(unsigned long long) * kVisitedWords, s));
      SX_HIP(sx_kde_cutoff_gather(k->D, adaptive, k->d_rows.get(), c.d_perm->get(), ntiles, c.d_sorted.get(),
                                  c.d_tile_box.get(), s));
      SX_HIP(sx_kde_pairs_cutoff(k->D, adaptive, k->d_pts.get(), k->pitch, c.d_sorted.get(), c.d_tile_box.get(),
                                 c.d_wave_box.get(), k->tiles_per_split, ntiles, k->nsplit, c.qcut, k->d_part.get(),
                                 c.d_visited.get(), s));
    } else {
      SX_HIP(sx_kde_pairs(k->D, adaptive, k->d_pts.get(), k->pitch, k->d_rows.get(), k->tiles_per_split, ntiles, k->nsplit,
                          k->d_part.get(), s));
    }
    SX_HIP(sx_kde_combine(k->d_part.get(), k->pitch, k->nsplit, k->npoints, k->d_codes.get(),
                          c.on() ? c.d_inv.get() : nullptr, a.norm, k->prefactor, k->pdf + k->pdf_off,
                          (long)k->pdf_stride, s));
  }
  k->cut.last_cut = lookup && k->cut.on();
  k->cut.last_possible = k->cut.last_cut ? (unsigned long long)k->cut.live_waves * (k->npad / SXMC_KDE_TILE) : 0ull;
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
int sxmc_kde_sample_total(sxmc_kde_t k, unsigned long long* total) {
  SX_REQUIRE(k && total, "null argument");
  *total = k->weighted() ? k->mult_total : (unsigned long long)k->nsamples;
  return SXMC_OK;
}
int sxmc_kde_get_sample_multiplicities(sxmc_kde_t k, unsigned* out, size_t n, int* is_set) {
  SX_REQUIRE(k && (out || n == 0), "null argument");
  if (is_set) *is_set = k->weighted() ? 1 : 0;
  if (!out && n == 0) return SXMC_OK;   // (the question alone: are any set?)
  SX_REQUIRE(n == k->nsamples, "sample multiplicities buffer size mismatch");
  if (!k->weighted()) std::fill(out, out + n, 1u);   // (none set: every row counts once)
  else std::copy(k->mult->begin(), k->mult->end(), out);
  return SXMC_OK;
}
int sxmc_kde_effective_samples(sxmc_kde_t k, double* n_eff) {
  SX_REQUIRE(k && n_eff, "null argument");
  *n_eff = k->weighted() ? k->n_eff : (double)k->n_inside;
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
    if (!k->cut.d_perm) {
      if (int rc_ = cutoff_sample_order(k)) return rc_;
    }
    if (int rc_ = cutoff_buffers(k)) return rc_;
  }
  const bool replan = k->has_points && (R > 0) != k->cut.points_sorted;
  k->cut.cutoff = R;
  k->cut.qcut = sxkde::cutoff_qcut(R);
  if (replan) return plan_points(k);
  return SXMC_OK;
}
int sxmc_kde_cutoff(sxmc_kde_t k, double* R) {
  SX_REQUIRE(k && R, "null argument");
  *R = k->cut.cutoff;
  return SXMC_OK;
}
int sxmc_kde_cutoff_stats(sxmc_kde_t k, unsigned long long* tiles_visited, unsigned long long* tiles_possible) {
  SX_REQUIRE(k && tiles_visited && tiles_possible, "null argument");
  *tiles_visited = 0;
  *tiles_possible = 0;
  if (!k->evaluated || !k->cut.last_cut) return SXMC_OK;
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  std::vector<unsigned long long> counters(kVisitedWords);
  SX_HIP(hipMemcpy(counters.data(), k->cut.d_visited.get(), sizeof(unsigned long long) * kVisitedWords, hipMemcpyDeviceToHost));
  for (int c = 0; c < sxkde::kCutCounters; c++) *tiles_visited += counters[(size_t)c * sxkde::kCutCounterStride];
  *tiles_possible = k->cut.last_possible;
  return SXMC_OK;
}
int sxmc_kde_cutoff_boxes(sxmc_kde_t k, float* tile_boxes, size_t ntile_floats, float* wave_boxes, size_t nwave_floats) {
  SX_REQUIRE(k && tile_boxes && wave_boxes, "null argument");
  if (!k->cut.on() || !k->has_points || !k->cut.points_sorted) {
    return fail(SXMC_ERR_STATE, "EvalKernel: no boxes without a cutoff and evaluation points");
  }
  SX_REQUIRE(ntile_floats == k->npad / SXMC_KDE_TILE * (size_t)sxkde::kCutBox &&
                 nwave_floats == k->pitch / sxkde::kCutWave * (size_t)sxkde::kCutWaveBox,
             "cutoff box buffer size mismatch");
  if (int rc_ = order_after_caller(k)) return rc_;
  SX_HIP(hipStreamSynchronize(k->h->stream));
  SX_HIP(hipMemcpy(tile_boxes, k->cut.d_tile_box.get(), sizeof(float) * ntile_floats, hipMemcpyDeviceToHost));
  SX_HIP(hipMemcpy(wave_boxes, k->cut.d_wave_box.get(), sizeof(float) * nwave_floats, hipMemcpyDeviceToHost));
  return SXMC_OK;
}
int sxmc_kde_pair_split(sxmc_kde_t k, int* nsplit, unsigned* tiles_per_split) {
  SX_REQUIRE(k && nsplit && tiles_per_split, "null argument");
  if (!k->has_points) return fail(SXMC_ERR_STATE, "EvalKernel: no pair split without evaluation points");
  *nsplit = k->nsplit;
  *tiles_per_split = k->tiles_per_split;
  return SXMC_OK;
}
int sxmc_kde_npoints(sxmc_kde_t k, size_t* v) {
  SX_REQUIRE(k && v, "null argument");
  *v = k->has_points ? k->npoints : 0;
  return SXMC_OK;
}

}  // extern "C"

