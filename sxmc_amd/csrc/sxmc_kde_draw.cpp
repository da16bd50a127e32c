// sxmc_kde_draw.cpp -- what reads the rows the last evaluation of a pdfz::EvalKernel left (sxmc_kde.cpp): the list of
// its in-domain rows, the events drawn from them (sxmc_kde_random_sample) and the projection onto one observable
// (sxmc_kde_project).  The kernels are in kde_kernels.hip, the contract in include/sxmc_hip.h.
#include "sxmc_kde_state.h"

#include <limits>

using namespace sxhost;

namespace {

// What a look at the last evaluation's rows needs first: an evaluation, the caller's stream settled, d_flag and the
// scan's scratch.
int kde_draw_ready(sxmc_kde_t k) {
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
  return SXMC_OK;
}

// Lists the live rows of the last evaluation (weight > 0: inside the domain, and of multiplicity > 0 where there are
// multiplicities) on the evaluator's stream and returns their count n (without multiplicities the norm of that
// evaluation): after it, d_flag + 2 npad holds their row numbers in table order.
int kde_compact(sxmc_kde_t k, unsigned& n) {
  if (int rc_ = kde_draw_ready(k)) return rc_;
  const hipStream_t s = k->h->stream;
  unsigned* flag = k->d_flag.get();
  unsigned* pos = flag + k->npad;
  unsigned* idx = pos + k->npad;
  SX_HIP(sx_kde_compact(k->d_rows.get(), k->rowlen(), k->npad, flag, pos, idx, k->d_scan_temp.get(), k->scan_temp_bytes, s));
  SX_HIP(hipMemcpyAsync(&n, pos + (k->npad - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  return SXMC_OK;
}

// With multiplicities: the inclusive prefix sum of the live rows' multiplicities over all npad rows, in table order, on
// the evaluator's stream, and its last entry T (= the norm of the last evaluation): after it, d_flag + npad holds the sum.
int kde_weighted_scan(sxmc_kde_t k, unsigned& total) {
  if (int rc_ = kde_draw_ready(k)) return rc_;
  const hipStream_t s = k->h->stream;
  unsigned* flag = k->d_flag.get();
  unsigned* cum = flag + k->npad;
  SX_HIP(sx_kde_weighted_scan(k->d_rows.get(), k->rowlen(), k->npad, k->mult_ptr(), flag, cum, k->d_scan_temp.get(),
                              k->scan_temp_bytes, s));
  SX_HIP(hipMemcpyAsync(&total, cum + (k->npad - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s));
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
  unsigned n = 0;   // the in-domain rows, or (with multiplicities) their multiplicities' total
  int rc = k->weighted() ? kde_weighted_scan(k, n) : kde_compact(k, n);
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
  if (k->weighted()) {
    SX_HIP(sx_kde_sample_weighted(D, k->d_rows.get(), k->d_lambda.get(), k->d_flag.get() + k->npad, n, k->npad, g, seed,
                                  nobserved, d_out, d_exhausted, k->h->stream));
  } else {
    const unsigned* idx = k->d_flag.get() + 2 * k->npad;
    SX_HIP(sx_kde_sample(D, k->d_rows.get(), k->d_lambda.get(), idx, n, g, seed, nobserved, d_out, d_exhausted, k->h->stream));
  }
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
  sxkde::project_split(k->npad, (unsigned long long)nbins, a.rows_per_split, a.nsplit, a.pitch);
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
  SX_HIP(sx_kde_project(k->d_rows.get(), a, k->mult_ptr(), k->d_proj.get(), d_count, d_prob, s));
  SX_HIP(hipMemcpyAsync(h_prob, d_prob, sizeof(double) * (size_t)nbins, hipMemcpyDeviceToHost, s));
  SX_HIP(hipStreamSynchronize(s));
  return SXMC_OK;
}

}  // extern "C"
