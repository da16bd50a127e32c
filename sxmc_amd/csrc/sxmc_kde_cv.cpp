// sxmc_kde_cv.cpp -- bandwidth cross-validation of pdfz::EvalKernel (sxmc_kde_cv_scores, sxmc_kde_cv_select; the host
// arithmetic in kde_cv.h): the untransformed in-domain rows are read back from the table, the candidates' constants made
// on the host, the weights, the pair sums and the logarithms on the device (kde_cv_* of kde_kernels.hip), the m
// logarithms of a candidate added here in table order.  The evaluator (sxmc_kde.cpp) keeps sigma, its scales and the
// in-domain count from creation for it; its bandwidths never change.
#include "sxmc_kde_state.h"

#include "kde_cv.h"

using namespace sxhost;

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
  std::vector<float> cols;
  if (int rc_ = table_columns(k, cols)) return rc_;
  const std::vector<size_t> inside = sxkde::rows_inside(cols.data(), 1, n, n, D, k->h->lower.data(), k->h->upper.data());
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

// The leave-one-out score of a table with multiplicities is a law of its own (a row's own copies, its error bound): not
// built, refused by name.
int cv_refuse_weighted(sxmc_kde* k) {
  if (!k->weighted()) return SXMC_OK;
  return fail(SXMC_ERR_STATE, "EvalKernel: cross-validation of an evaluator with sample multiplicities is not built (the "
                              "weighted leave-one-out score): choose the bandwidth scales on the unweighted table");
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
  if (int rc_ = cv_refuse_weighted(k)) return rc_;
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
  if (int rc_ = cv_refuse_weighted(k)) return rc_;
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
