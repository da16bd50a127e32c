// sxmc_launch_plan.cpp -- a group's launch plan: device-resident tables (bucketed copies, codes, sparse structures), launch classes,
// partitions, launch shapes; refresh when bindings or settings change; event classes; the fill launches.
#include "sxmc_host.h"

using namespace sxhost;

namespace sxhost {

using sxplan::apportion_workgroups;

// a host vector's copy on the device, in an empty buffer allocated for at least `room` elements
template <typename T>
hipError_t upload(const std::vector<T>& v, DeviceBuffer<T>& d, size_t room = 0) {
  const hipError_t e = (hipError_t)d.alloc(std::max(v.size(), room));
  return (e != hipSuccess || v.empty()) ? e : hipMemcpy(d.get(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

// Slot assignment: observables first (slot k = field k), then every other field a systematic
// references, ascending.
void member_slots(const sxmc_hist* h, std::vector<int>& slot_col) {
  slot_col.clear();
  for (int k = 0; k < h->nobs; k++) slot_col.push_back(k);
  std::vector<int> extra;
  for (const HostSyst& s : h->systs) {
    if (s.obs >= h->nobs) extra.push_back(s.obs);
    if (s.type == SXMC_SYST_RESOLUTION_SCALE && s.extra_field >= h->nobs) extra.push_back(s.extra_field);
  }
  std::sort(extra.begin(), extra.end());
  extra.erase(std::unique(extra.begin(), extra.end()), extra.end());
  for (int c : extra) slot_col.push_back(c);
}

int slot_of(const std::vector<int>& slot_col, int field) {
  for (size_t k = 0; k < slot_col.size(); k++)
    if (slot_col[k] == field) return (int)k;
  return 0;
}

void reset_bucket_tables(sxmc_hist* h) {
  h->d_bdir.reset();
  h->d_btkeys.reset();
  h->d_btslot.reset();
  h->btab_valid = false;
}

void free_sparse(sxmc_hist* h) {
  reset_bucket_tables(h);
  h->d_cnt.reset();
  h->d_read_slot.reset();
  h->d_filter.reset();
  h->d_table.reset();
  h->d_coarse.reset();
  h->ntargets = 0;
  h->targets.clear();
  h->h_read_slot.clear();
}

using sxplan::ceil_log2;

// Sparse-counting structures of one evaluator from its event bins (host side, once per SetEvalPoints).
int build_sparse(sxmc_hist* h, const std::vector<int>& rb) {
  free_sparse(h);
  sxplan::SparseTables st;
  sxplan::build_sparse_tables(rb, st);   // (sxmc_plan.h: targets, slots, filters, table)
  const std::vector<unsigned>&targets = st.targets, &filter = st.filter, &table = st.table, &coarse = st.coarse;
  const std::vector<int>& slot = st.slot;
  const size_t T = targets.size();
  const int cbits = st.cbits, fbits = st.fbits, tbits = st.tbits;
  SX_BUF(h->d_cnt.alloc(std::max<size_t>(T, 4)));
  SX_HIP(hipMemset(h->d_cnt.get(), 0, sizeof(unsigned) * std::max<size_t>(T, 4)));
  SX_HIP(upload(slot, h->d_read_slot, 1));
  SX_HIP(upload(filter, h->d_filter));
  SX_HIP(upload(table, h->d_table));
  SX_HIP(upload(coarse, h->d_coarse));
  h->h_read_slot = slot;
  h->coarse_shift = 32 - cbits;
  h->ntargets = (int)T;
  h->targets = targets;
  h->filter_shift = 32 - fbits;
  h->table_shift = 32 - tbits;
  return SXMC_OK;
}

// The sparse flavour of a member's descriptor: counters instead of the histogram, slots instead of bins.
void make_sparse_desc(const sxmc_hist* h, SxSignalDesc& d) {
  d.sparse_real_nbins = h->total_nbins;
  d.bins = h->d_cnt.get();
  d.total_nbins = std::max(h->ntargets, 1);
  d.read_bins = h->d_read_slot.get();
  d.sparse_filter = h->d_filter.get();
  d.sparse_table = h->d_table.get();
  d.sparse_filter_shift = h->filter_shift;
  d.sparse_table_shift = h->table_shift;
  d.sparse_coarse = h->d_coarse.get();
  d.sparse_coarse_shift = h->coarse_shift;
}

int fill_desc(const sxmc_hist* h, SxSignalDesc& d) {
  std::memset(&d, 0, sizeof(d));
  std::vector<int> slot_col;
  member_slots(h, slot_col);
  d.cols = h->store->d_cols.get();
  d.col_pitch = h->pitch;
  d.nsamples = h->nsamples;
  d.nvec = h->nvec;
  d.bins = h->d_bins.get();
  d.norm = h->norm ? h->norm + h->norm_off : nullptr;
  d.total_nbins = h->total_nbins;
  d.nobs = h->nobs;
  d.nslot = (int)slot_col.size();
  d.nsyst = (int)h->systs.size();
  d.param_stride = h->par_stride;
  d.params = h->params ? h->params + h->par_off : nullptr;
  for (int k = 0; k < d.nslot; k++) d.slot_col[k] = slot_col[k];
  for (int k = 0; k < h->nobs; k++) {
    d.nbins[k] = h->nbins[(size_t)k];
    d.bin_stride[k] = h->stride[k];
    d.lower[k] = h->lower[k];
    d.upper[k] = h->upper[k];
    d.scale[k] = h->scale[k];
  }
  int ncoef = 0;
  for (int s = 0; s < d.nsyst; s++) {
    const HostSyst& hs = h->systs[s];
    SxSystOp& op = d.syst[s];
    op.type = (short)hs.type;
    op.obs_slot = (short)slot_of(slot_col, hs.obs);
    op.extra_slot = (short)(hs.type == SXMC_SYST_RESOLUTION_SCALE ? slot_of(slot_col, hs.extra_field) : 0);
    op.npars = (short)hs.pars.size();
    op.coef_start = (short)ncoef;
    for (size_t i = 0; i < hs.pars.size(); i++) {
      op.pars[i] = hs.pars[i];
      if (ncoef < 64) d.coef_par[ncoef] = hs.pars[i];
      ncoef++;
    }
  }
  d.ncoef = ncoef;
  d.read_bins = h->has_points ? h->d_read_bins.get() : nullptr;
  d.npoints = h->has_points ? h->npoints : 0;
  d.pdf_out = h->pdf ? h->pdf + h->pdf_off : nullptr;
  d.pdf_stride = h->pdf_stride;
  d.bin_volume = h->bin_volume;
  return SXMC_OK;
}

// strata of x - t inside a bucket of a boxed table (SXMC_BOX_STRATA, measurement build: 1 .. 16).  More strata make the
// boxes narrower in x - t and wider in x: at BASELINE config 3 a CPU model of the layout puts the granules whose box
// straddles an edge at 0.8 / 1.5 / 2.9 % for 1 / 2 / 4 strata at a resolution parameter of 0, 4 / 3.2 / 3.6 % at 0.01 and
// 17 / 10 / 7.8 % at 0.05 (its prior width).  Measured on the walk of the bench (one box, alternating,
// profiles/r05_boxed_strata.log): 65.2-65.9 us for 1 or 2 strata, 67.3 for 4, 71.4 for 8.  Two.
int box_strata() {
  static const int n = [] {
    const char* e = measure_env("SXMC_BOX_STRATA");
    return e ? std::min(std::max(std::atoi(e), 1), 16) : 2;
  }();
  return n;
}

// The rows of member `h`'s table sorted by their bin indices in the observables of `mask` (those no systematic
// writes) and cut into 256-row granules, bucket by bucket.  Fetched from the table's cache or built; *out =
// nullptr when bucketing does not pay for this table.  d_full_desc: the member's descriptor on the device.
// `ordered` >= 0: inside every bucket the rows are in ascending order of that observable's raw value (NaN last).
int get_bucket_sort(sxmc_hist* h, const SxSignalDesc* d_full_desc, unsigned mask, int ordered,
                    const SampleStore::BucketSort** out, int box_truth = -1) {
  *out = nullptr;
  SampleStore& st = *h->store;
  std::lock_guard<std::mutex> lock(st.pre_mutex);
  if (SampleStore::BucketSort* have = st.find_sort(mask, ordered, box_truth)) {
    *out = have->rejected ? nullptr : have;
    return SXMC_OK;
  }
  st.sorts.push_back(std::make_unique<SampleStore::BucketSort>());
  SampleStore::BucketSort* b = st.sorts.back().get();
  b->mask = mask;
  b->ordered = ordered;
  b->box_truth = box_truth;
  const size_t n = h->nsamples;
  if (n == 0 || n > 0x7FFFFF00ull) return SXMC_OK;

  // key space: mixed radix over the untouched observables, last one fastest, bases nbins + 1 (an index can
  // come out as nbins one ulp below the upper edge; such samples form buckets of their own)
  unsigned long long nkeys = 1;
  for (int k = h->nobs - 1; k >= 0; k--) {
    if (!((mask >> k) & 1u)) continue;
    b->radix[k] = (unsigned)nkeys;
    nkeys *= (unsigned long long)h->nbins[(size_t)k] + 1ull;
    if (nkeys > (1ull << 20)) return SXMC_OK;
  }
  const unsigned outside = (unsigned)nkeys;
  const int bits = ceil_log2((size_t)nkeys + 1);

  DeviceBuffer<unsigned> keys0, keys1, rows0, dfirst;   // (temporaries: freed on every way out)
  SX_BUF(keys0.alloc(n));
  SX_BUF(keys1.alloc(n));
  SX_BUF(rows0.alloc(n));
  SX_BUF(b->d_rows.alloc(n));
  SX_BUF(dfirst.alloc(nkeys + 1));
  SX_HIP(hipMemset(dfirst.get(), 0xFF, (nkeys + 1) * 4));
  const unsigned* order_rows = nullptr;
  DeviceBuffer<unsigned> rows1;
  if (ordered >= 0) {
    // rows by the ordered observable's value first; the stable sort by bucket below keeps that order inside a bucket
    SX_BUF(rows1.alloc(n));
    if (box_truth >= 0) {
      // BOXED observable: strata of x - t (their boundaries: quantiles, read off a first sort), x ascending inside
      const float* colx = st.d_cols.get() + (size_t)ordered * h->pitch;
      const float* colt = st.d_cols.get() + (size_t)box_truth * h->pitch;
      const int nstrata = box_strata();
      unsigned bounds[16] = {0};
      if (nstrata > 1) {
        SX_HIP(sx_box_keys(colx, colt, n, 1, 1, nullptr, keys0.get(), rows0.get(), nullptr));
        SX_HIP(sx_bucket_sort(keys0.get(), keys1.get(), rows0.get(), rows1.get(), n, 32,
                              nullptr));
        for (int k = 0; k + 1 < nstrata; k++) {
          SX_HIP(hipMemcpy(&bounds[k], keys1.get() + (size_t)((double)n * (k + 1) / nstrata), 4,
                           hipMemcpyDeviceToHost));
        }
      }
      SX_HIP(sx_box_keys(colx, colt, n, 2, nstrata, bounds, keys0.get(), rows0.get(), nullptr));
    } else {
      SX_HIP(sx_order_keys(st.d_cols.get() + (size_t)ordered * h->pitch, n, keys0.get(),
                           rows0.get(), nullptr));
    }
    SX_HIP(sx_bucket_sort(keys0.get(), keys1.get(), rows0.get(), rows1.get(), n, 32,
                          nullptr));
    order_rows = rows1.get();
  }
  SX_HIP(sx_bucket_keys(d_full_desc, n, mask, b->radix, outside, order_rows, keys0.get(), rows0.get(),
                        nullptr));
  SX_HIP(sx_bucket_sort(keys0.get(), keys1.get(), rows0.get(), b->d_rows.get(), n, bits, nullptr));
  SX_HIP(sx_bucket_first(keys1.get(), n, dfirst.get(), nullptr));
  std::vector<unsigned> first((size_t)nkeys + 1);
  SX_HIP(hipMemcpy(first.data(), dfirst.get(), first.size() * 4, hipMemcpyDeviceToHost));

  // logical granules: bucket by bucket, each bucket padded to whole granules (sxmc_plan.h)
  sxplan::GranulePlan gp;
  sxplan::bucket_granules(first, outside, n, gp);
  if (!gp.worth_it) {  // mostly padding: not worth it
    b->d_rows.reset();
    return SXMC_OK;
  }
  b->lsrc = gp.lsrc;
  b->lvalid = gp.lvalid;
  b->lwhich = gp.lwhich;
  b->keys = gp.present;
  b->nkeys_total = outside;
  b->nkept = gp.kept;
  sxplan::bucket_key_offsets(gp.present, mask, b->radix, h->nbins.data(), h->stride.data(), h->nobs, b->key_pre);
  b->rejected = false;
  *out = b;
  return SXMC_OK;
}

// The bucketed COPY of the table for a sort: the columns `fields`, granule order transposed for `runs` runs --
// run r holds logical granules [r * T, (r + 1) * T), and the runs are interleaved granule by granule (physical
// p = t * runs + r), so that `runs` consumers that each walk one run read neighbouring addresses at the same
// time.  runs = 1: the sorted order itself.
int get_bucketed(sxmc_hist* h, const SampleStore::BucketSort* bs, const std::vector<int>& fields, int runs,
                 const SampleStore::Bucketed** out) {
  *out = nullptr;
  SampleStore& st = *h->store;
  std::lock_guard<std::mutex> lock(st.pre_mutex);
  if (SampleStore::Bucketed* have = st.find_bucketed(bs, fields, runs)) {
    if (!have->complete) return fail(SXMC_ERR_HIP, "an earlier attempt to lay this table out failed");
    *out = have;
    return SXMC_OK;
  }
  SX_REQUIRE(!fields.empty() && runs >= 1, "bad bucketed layout request");
  const bool pack_rows = bs->ordered >= 0 && h->total_nbins <= kLdsMaxBins;   // (fill_ordered_body, histogram in LDS)
  st.bucketed.push_back(std::make_unique<SampleStore::Bucketed>());
  SampleStore::Bucketed* b = st.bucketed.back().get();
  b->mask = bs->mask;
  b->fields = fields;
  b->runs = runs;
  b->sort = bs;
  sxplan::BucketedLayout lay;   // physical granule order for `runs` runs (sxmc_plan.h)
  sxplan::bucketed_layout(bs->lsrc, bs->lvalid, bs->lwhich, bs->keys, bs->key_pre, bs->nkeys_total, runs, pack_rows, lay);
  const size_t P = lay.P, A = lay.A;
  const std::vector<unsigned>&psrc = lay.psrc, &pvalid = lay.pvalid, &ppre = lay.ppre, &pkp = lay.pkp;
  b->ngranules = P;
  b->nkept = bs->nkept;
  b->pitch = std::max<size_t>(64, P * 256);
  DeviceBuffer<unsigned> dsrc, dvalid;   // (temporaries)
  SX_BUF(b->d_cols.alloc(b->pitch * fields.size()));
  SX_BUF(b->d_gpre.alloc(A));
  SX_BUF(b->d_gkp.alloc(2 * A));
  SX_HIP(hipMemcpy(b->d_gpre.get(), ppre.data(), sizeof(unsigned) * A, hipMemcpyHostToDevice));
  SX_HIP(hipMemcpy(b->d_gkp.get(), pkp.data(), sizeof(unsigned) * 2 * A, hipMemcpyHostToDevice));
  SX_BUF(dsrc.alloc(A ? A : 4));
  SX_BUF(dvalid.alloc(A ? A : 4));
  SX_HIP(hipMemcpy(dsrc.get(), psrc.data(), A * 4, hipMemcpyHostToDevice));
  SX_HIP(hipMemcpy(dvalid.get(), pvalid.data(), A * 4, hipMemcpyHostToDevice));
  SX_HIP(sx_bucket_gather(st.d_cols.get(), h->pitch, (int)fields.size(), fields.data(), bs->d_rows.get(), dsrc.get(),
                          dvalid.get(), P, b->d_cols.get(), b->pitch, nullptr));
  if (bs->ordered >= 0 && bs->box_truth >= 0) {
    // the boxed observable's column is the last of `fields`, its truth field the one before (sxplan::compact_slots)
    SX_REQUIRE(fields.size() >= 2, "a boxed layout streams its observable and the truth field");
    SX_BUF(b->d_gbox.alloc(4 * A));
    SX_HIP(hipMemset(b->d_gbox.get(), 0xFF, sizeof(float) * 4 * A));   // (NaN: a granule never written is left to the float columns)
    SX_HIP(sx_bucket_boxes(b->d_cols.get() + (fields.size() - 1) * b->pitch, b->d_cols.get() + (fields.size() - 2) * b->pitch,
                           dvalid.get(), P, b->d_gbox.get(), nullptr));
    {   // mean extents of the finite boxes (what a dual launch estimates the share of straddling granules from)
      std::vector<float> hb(4 * P);
      if (P) SX_HIP(hipMemcpy(hb.data(), b->d_gbox.get(), sizeof(float) * 4 * P, hipMemcpyDeviceToHost));
      // (the mean of the lower nine tenths: the granules of a bucket's thin tails are wide whatever the layout and are
      // few; they straddle an edge at any parameters and say nothing about the rest)
      std::vector<double> ex, et;
      for (size_t p = 0; p < P; p++) {
        const float x0 = hb[4 * p], x1 = hb[4 * p + 1], t0 = hb[4 * p + 2], t1 = hb[4 * p + 3];
        if (!(std::isfinite(x0) && std::isfinite(x1) && std::isfinite(t0) && std::isfinite(t1))) continue;
        ex.push_back((double)x1 - (double)x0);
        et.push_back((double)t1 - (double)t0);
      }
      auto trimmed = [](std::vector<double>& v) {
        if (v.empty()) return 0.0;
        std::sort(v.begin(), v.end());
        const size_t keep = std::max<size_t>(1, v.size() * 9 / 10);
        double sum = 0;
        for (size_t i = 0; i < keep; i++) sum += v[i];
        return sum / (double)keep;
      };
      b->box_dx = trimmed(ex);
      b->box_dt = trimmed(et);
    }
  } else if (bs->ordered >= 0) {
    // the ordered observable's column is the last of `fields` (sxplan::compact_slots)
    SX_BUF(b->d_gedge.alloc(2 * A));
    SX_HIP(hipMemset(b->d_gedge.get(), 0, sizeof(float) * 2 * A));
    SX_HIP(sx_bucket_edges(b->d_cols.get() + (fields.size() - 1) * b->pitch, dvalid.get(), P, b->d_gedge.get(), nullptr));
  }
  SX_HIP(hipDeviceSynchronize());
  b->complete = true;
  *out = b;
  return SXMC_OK;
}

// CODES (fill_ordered_body): the streamed fields of a bucketed copy with an ordered observable once more, as 16-bit
// codes inside a window per field, two fields to a word.  `cd`: the member as its fill sees it -- slots 0 .. nobs-1 are
// observables (their domains centre the windows), the others fields only read.  The window of an observable is its
// finite range in the table cut to the domain widened by its own width on either side (a value further out needs a
// scale or shift of the order of the whole domain to come back in: its row is marked "ask the exact columns"
// instead); the window of a field that is only read is its finite range, cut to three such widths around the
// observables' windows when they overlap at all.  Built once per copy; left out (d_qcol stays null) when more than
// 2 % of the rows would ask the exact columns: such a table gains nothing.
bool codes_enabled(const PlanConfig& cfg) {
  if (cfg.codes >= 0) return cfg.codes != 0;
  static const bool on = [] {
    const char* e = std::getenv("SXMC_CODES");
    return !e || std::atoi(e) != 0;
  }();
  return on;
}

int get_bucket_codes(sxmc_hist* h, const SampleStore::Bucketed* bkc, const SxSignalDesc& cd) {
  SampleStore& st = *h->store;
  std::lock_guard<std::mutex> lock(st.pre_mutex);
  SampleStore::Bucketed* b = const_cast<SampleStore::Bucketed*>(bkc);
  if (b->codes_tried) return SXMC_OK;
  b->codes_tried = true;
  // (an ordered copy: every field but the ordered observable's, the last; an unordered one -- the sparse counting over
  // runs -- : every field)
  const bool boxed = b->sort && b->sort->ordered >= 0 && b->sort->box_truth >= 0;
  const int nq = (int)b->fields.size() - ((b->sort && b->sort->ordered >= 0) ? 1 : 0) - (boxed ? 1 : 0);
  // (below 2^22 granules a unit's byte offset into a column of codes fits 32 bits, and a unit number 28: what the
  // ordered kernel's addressing and its queue entries assume)
  if ((boxed ? nq != 1 : nq < 2) || nq > SXMC_MAX_QSLOTS || b->ngranules == 0 || b->ngranules >= ((size_t)1 << 22) || !b->sort) {
    return SXMC_OK;
  }
  const unsigned long long n = (unsigned long long)b->ngranules * 256ull;
  float mm[2 * SXMC_MAX_NFIELDS];
  SX_HIP(sx_column_minmax(b->d_cols.get(), b->pitch, nq, n, mm, nullptr));
  sxplan::CodeWindows cw;   // (sxmc_plan.h: pure, tested without a device)
  sxplan::code_windows(mm, nq, cd.nobs, cd.lower, cd.upper, cw);
  for (int m = 0; m < nq; m++) {
    b->qbase[m] = cw.base[(size_t)m];
    b->qstep[m] = cw.step[(size_t)m];
  }
  // Do they pay?  A sample is ambiguous when a bin coordinate lies within ~half a code step (in bins) of an integer:
  // about sum_k nbins_k * step_k / (upper_k - lower_k) of the samples for systematics near their means.  Beyond 2 in
  // 10^3, four 256-sample units in ten hold an ambiguous sample and the queues' traffic eats what the codes save
  // (measured at 200 bins per observable: slower than the float stream): such tables keep their float stream.
  double ambiguous = 0;
  for (int m = 0; m < nq && m < cd.nobs; m++) ambiguous += (double)cd.nbins[m] * cw.step[(size_t)m] / (cd.upper[m] - cd.lower[m]);
  static const bool gate_lifted = [] {   // (SXMC_CODES_GATE=1, measurement build: profiles/r04b_codes_gate_probe.log)
    const char* e = measure_env("SXMC_CODES_GATE");
    return e && e[0] == '1';
  }();
  if (!(ambiguous <= 2e-3) && !gate_lifted) return SXMC_OK;
  // (the codes are an extra: a table they do not fit beside -- +4 bytes per row and pair of fields -- keeps its float stream)
  // (elements are words: a boxed table's 16-bit codes take half a word per row, and the pitch is even)
  if (b->d_qcol.alloc(boxed ? b->pitch / 2 : b->pitch * (size_t)((nq + 1) / 2)) != 0) {
    (void)hipGetLastError();
    return SXMC_OK;
  }
  unsigned long long tally[2] = {0, 0};
  b->q16 = boxed;
  hipError_t e = boxed ? sx_column_codes16(b->d_cols.get(), b->qbase[0], b->qstep[0], n, reinterpret_cast<unsigned short*>(b->d_qcol.get()),
                                           tally, nullptr)
                       : sx_column_codes(b->d_cols.get(), b->pitch, nq, b->qbase, b->qstep, n, b->d_qcol.get(), tally, nullptr);
  if (e != hipSuccess || (double)tally[0] > 0.02 * (double)std::max<size_t>(b->nkept, 1)) {
    b->d_qcol.reset();
    if (e != hipSuccess) return fail(SXMC_ERR_HIP, std::string("codes of a bucketed table: ") + hipGetErrorString(e));
    return SXMC_OK;
  }
  b->nq = nq;
  b->q_exact_rows = tally[0];
  b->q_never_rows = tally[1];
  return SXMC_OK;
}


// The evaluator's event bins grouped by the buckets of a sort (fill_sparse_kernel): per bucket key an
// open-addressing table keyed by the event bin's index contribution of the WRITTEN observables (flat index minus
// the bucket's offset, canonical decomposition), value = the event bin's counter slot (its rank among the sorted
// distinct event bins, as in build_sparse).  Rebuilt when the evaluation points or the untouched set change.
int build_bucket_tables(sxmc_hist* h, const SampleStore::BucketSort* bs) {
  if (h->btab_valid && h->btab_mask == bs->mask && h->btab_points_version == h->points_version) return SXMC_OK;
  reset_bucket_tables(h);
  sxplan::BucketTables bt;   // directory + per-bucket tables of the event bins (sxmc_plan.h)
  sxplan::bucket_tables(bs->nkeys_total, bs->mask, bs->radix, h->nbins.data(), h->stride.data(), h->nobs, h->targets, bt);
  const std::vector<unsigned>&dir = bt.dir, &tkeys = bt.tkeys, &tslot = bt.tslot;
  SX_HIP(upload(dir, h->d_bdir));
  SX_HIP(upload(tkeys, h->d_btkeys, 4));
  SX_HIP(upload(tslot, h->d_btslot, 4));
  h->btab_mask = bs->mask;
  h->btab_points_version = h->points_version;
  h->btab_valid = true;
  return SXMC_OK;
}


// The whole step in one launch (fill_step_kernel), when asked for: its role workgroups carry the fill's LDS allotment
// and need 16 KB of their own beside it, which the plan of an ordered fill then leaves free.
bool fused_step_requested(const PlanConfig& cfg) {
  static const int env_default = [] {
    const char* e = std::getenv("SXMC_FUSED_STEP");
    return (e && e[0] == '1') ? 1 : 0;
  }();
  return (cfg.fused < 0 ? env_default : cfg.fused) != 0;
}

// ---- the launch plan, step by step.  What a step decides without the device is in sxmc_plan.h (syst_use, choose_ordered,
// choose_boxed, compact_slots, prebin_columns, ordered_lds_layout); here: the kernel tables, the device's tables, uploads.
// A step reads the group `g` for its members and the descriptors both forms share and `cfg` for the settings of the form it
// plans; what it produces goes into the LaunchPlan (or the class of it) it is handed, never into the group (but rtc_note).

// What a step of the plan found it cannot lay out: plan_form runs the pass again without that form.
enum class Blocked { none, order, box };

inline bool is_boxed(const LaunchClass& c) { return sx_form_boxed(c.shape.form); }
inline bool is_ordered(const LaunchClass& c) { return sx_form_ordered(c.shape.form); }   // (the LDS layout, shapes and partition of the ordered form)
inline bool is_bucketed(const LaunchClass& c) { return sx_form_bucketed(c.shape.form); }

// One member's part of the plan: the form its table takes and the kernel that runs it.
struct MemberPlan {
  // the key of its launch class (find_class): shape.nobs / nslot / lds_hist / form / rtc_fill / rtc_sparse, prog,
  // prog_simple, pre_mask, runs_mode; with it shape.static_prog and the boxed form's slots.  find_class moves it in as
  // the new class: set nothing else on it.
  LaunchClass cls;
  // bucketed forms: what to lay out once the class's shape is known
  const SampleStore::BucketSort* sort = nullptr;
  std::vector<int> fields;
  SxSignalDesc desc;                  // the member as its fill launch sees it
};

// is there a kernel for this specialisation?  *fn: the run-time one, or null for a built-in one (sp: its index)
bool have_kernel(sxmc_group* g, const PlanConfig& cfg, int lds_hist, int nobs, int nslot, int form, int runs,
                 const std::vector<unsigned>& words, int sp, void** fn) {
  *fn = nullptr;
  if (sx_fill_supports(sp, form, lds_hist, runs)) return true;
  if (!cfg.rtc) return false;
  SxRtcSpec k{};
  k.nobs = nobs;
  k.nslot = nslot;
  k.lds_hist = lds_hist;
  k.form = form;
  k.sparse_runs = runs;
  k.nops = (int)words.size();
  for (size_t q = 0; q < words.size(); q++) k.ops[q] = words[q];
  std::string err;
  *fn = sx_rtc_get(k, &err);
  if (!*fn) g->rtc_note = err;
  return *fn != nullptr;
}

// ---- bucketed table: the observables no systematic writes become a per-granule bin offset and the
// fill sees the lower-dimensional problem of the ones that are written.  With an ORDERED observable (written
// only by monotone one-coefficient systematics, read by nothing): that one too is a per-granule constant,
// worked out per evaluation from the granule's end values, except in the granules that straddle a bin edge.
// box_truth >= 0: `ordered` is a BOXED observable (fill_boxed_kernel) and box_truth the slot of its truth field.
// mp.sort stays null where the form does not apply: no such shape, no kernel, or bucketing does not pay for the table.
int plan_bucketed(sxmc_group* g, const PlanConfig& cfg, LaunchPlan& plan, int i, const sxplan::SystUse& use, int ordered,
                  int box_truth, MemberPlan& mp) {
  mp = MemberPlan{};
  LaunchClass& k = mp.cls;
  sxmc_hist* h = g->members[(size_t)i];
  const SxSignalDesc& d = g->h_descs[(size_t)i];
  const int lds_hist = k.shape.lds_hist = h->total_nbins <= kLdsMaxBins ? 1 : 0;
  const sxplan::CompactSlots cs = sxplan::compact_slots(d, use, ordered, box_truth, lds_hist != 0);
  if (!cs.shape_ok || (ordered < 0 && !sx_fill_has_specialization(cs.nobs2, (int)cs.fields.size()))) return SXMC_OK;
  SxSignalDesc cd;
  sxplan::compact_desc(d, cs.keep, cs.nobs2, cd, ordered);
  const std::vector<unsigned> prog2 = sxplan::prog_words(cd);
  const int form = box_truth >= 0 ? kFormBoxed : ordered >= 0 ? kFormOrdered : kFormBucketed;
  const int sp = sx_fill_find_program(form, cd.nobs, cd.nslot, (int)prog2.size(), prog2.data());
  if (!have_kernel(g, cfg, lds_hist, cd.nobs, cd.nslot, form, 0, prog2, sp, &k.shape.rtc_fill)) return SXMC_OK;
  const SampleStore::BucketSort* bs = nullptr;
  int rc = get_bucket_sort(h, g->d_descs.get() + i, cs.mask, ordered, &bs, box_truth >= 0 ? d.slot_col[box_truth] : -1);
  if (rc) return rc;
  if (!bs) {
    k.shape.rtc_fill = nullptr;
    return SXMC_OK;
  }
  mp.desc = cd;     // (columns, unit count and granule table: once the layout is chosen)
  mp.sort = bs;
  mp.fields = cs.fields;
  // histograms beyond LDS, evaluated at data events: per-wave runs + event bins grouped by bucket
  const bool narrow = sxplan::narrow_for_runs(d);
  k.runs_mode = !lds_hist && narrow && h->has_points && h->d_table && box_truth < 0 &&
                have_kernel(g, cfg, lds_hist, cd.nobs, cd.nslot, form, 1, prog2, sp, &k.shape.rtc_sparse);
  if (!lds_hist && !narrow && h->has_points && h->d_table) {
    // (a regression on very large histograms must be visible: sxmc_group_launch_info prints this)
    plan.note = "histogram with a bin count or stride of 2^23 or more: the sparse counting over runs (one signed "
                   "24-bit multiply-add per index) does not apply, the general sparse path runs instead";
  }
  if (k.runs_mode) {
    rc = build_bucket_tables(h, bs);
    if (rc) return rc;
  }
  k.shape.nobs = cd.nobs;
  k.shape.nslot = cd.nslot;
  k.prog = prog2;
  k.prog_simple = true;
  k.shape.static_prog = k.shape.rtc_fill ? -1 : sp;
  k.pre_mask = cs.pre_mask;
  k.shape.form = form;
  k.box_obs = box_truth >= 0 ? ordered : -1;
  k.box_truth = box_truth;
  return SXMC_OK;
}

// The table as it is: rows, or with the observables no systematic writes pre-binned.
// `weighted` (the member carries sample multiplicities): rows only, the straight-line kernel where the registry has a
// weighted one for the program, else the program decoded at run time by the weighted kernel of this (nobs, nslot) or the
// shape-agnostic one -- no run-time specialisation, nothing pre-binned.
MemberPlan plan_rows(sxmc_group* g, const PlanConfig& cfg, const SxSignalDesc& d, const sxplan::SystUse& use, int lds_hist,
                     bool weighted = false) {
  MemberPlan mp{};
  LaunchClass& k = mp.cls;
  mp.desc = d;
  k.shape.lds_hist = lds_hist;
  const bool spec = sx_fill_has_specialization(d.nobs, d.nslot) && d.ncoef <= 64;
  k.shape.nobs = spec ? d.nobs : 0;
  k.shape.nslot = spec ? d.nslot : 0;
  k.prog = sxplan::prog_words(d);
  if (weighted) {
    // (the registry's weighted straight-line kernels, where the program has them; the class is then keyed by it)
    const int wsp = (spec && use.specialisable)
                        ? sx_fill_find_program(kFormRows, k.shape.nobs, k.shape.nslot, (int)k.prog.size(), k.prog.data())
                        : -1;
    k.shape.weighted = 1;
    k.prog_simple = sx_fill_weighted_supports(wsp, lds_hist);
    k.shape.static_prog = k.prog_simple ? wsp : -1;
    return mp;
  }
  const int sp = (spec && use.specialisable)
                     ? sx_fill_find_program(kFormRows, k.shape.nobs, k.shape.nslot, (int)k.prog.size(), k.prog.data())
                     : -1;
  k.prog_simple = spec && use.specialisable &&
                  have_kernel(g, cfg, lds_hist, k.shape.nobs, k.shape.nslot, kFormRows, 0, k.prog, sp, &k.shape.rtc_fill);
  k.shape.static_prog = (k.prog_simple && !k.shape.rtc_fill) ? sp : -1;
  // pre-binning: observables that no systematic writes (built-in programs only; bucketing covers the rest)
  if (cfg.prebin && sx_fill_supports(k.shape.static_prog, kFormPre1, lds_hist, 0)) {   // (1 byte: so 2 bytes)
    const sxplan::PrebinColumns pre = sxplan::prebin_columns(d, use);
    k.pre_mask = pre.mask;
    k.shape.form = pre.width;   // (kFormPre1 / kFormPre2 ARE the column's bytes per sample; 0: nothing to pre-bin)
  }
  return mp;
}

// The form member i's table takes: boxed, ordered, bucketed, pre-binned or rows -- the first that applies, pays and
// has a kernel.
int plan_member(sxmc_group* g, const PlanConfig& cfg, LaunchPlan& plan, const DeviceProps& props, int i, MemberPlan& mp) {
  sxmc_hist* h = g->members[(size_t)i];
  const SxSignalDesc& d = g->h_descs[(size_t)i];
  const int lds_hist = h->total_nbins <= kLdsMaxBins ? 1 : 0;
  const sxplan::SystUse use = sxplan::syst_use(d);
  if (h->mult) {   // (no bucketed, ordered or boxed table with a permuted multiplicity column, no codes: rows)
    mp = plan_rows(g, cfg, d, use, lds_hist, true);
    return SXMC_OK;
  }
  if (cfg.bucket && d.nsyst > 0 && use.specialisable) {
    const bool runs_possible = !plan.order_blocked && h->has_points && h->d_table && (int)g->members.size() <= props.cus;
    const int ordered = sxplan::choose_ordered(d, use, cfg.order, lds_hist != 0, runs_possible);
    // (the boxed form: beside the ordered one, codes on)
    const bool box_on = cfg.box != 0 && !plan.box_blocked && cfg.order && lds_hist && codes_enabled(cfg);
    const sxplan::BoxChoice box = sxplan::choose_boxed(d, use, box_on ? cfg.box : 0, box_strata(), lds_hist != 0);
    int rc = SXMC_OK;
    mp = MemberPlan{};
    if (box.obs >= 0) rc = plan_bucketed(g, cfg, plan, i, use, box.obs, box.truth, mp);
    if (!rc && !mp.sort && ordered >= 0) {
      rc = plan_bucketed(g, cfg, plan, i, use, ordered, -1, mp);
      if (mp.sort && !lds_hist && !mp.cls.runs_mode) mp = MemberPlan{};   // (no kernel for the runs: the unordered layout has the filter path)
    }
    if (!rc && !mp.sort) rc = plan_bucketed(g, cfg, plan, i, use, -1, -1, mp);
    if (rc || mp.sort) return rc;
  }
  mp = plan_rows(g, cfg, d, use, lds_hist);
  return SXMC_OK;
}

// The launch class of a member's plan: members with the same kernel and table form share a launch.
LaunchClass& find_class(LaunchPlan& plan, MemberPlan& mp, int threads) {
  const LaunchClass& k = mp.cls;
  for (LaunchClass& c : plan.classes) {
    if (c.shape.nobs == k.shape.nobs && c.shape.nslot == k.shape.nslot && c.shape.lds_hist == k.shape.lds_hist &&
        c.prog_simple == k.prog_simple && (!k.prog_simple || c.prog == k.prog) && c.pre_mask == k.pre_mask &&
        c.shape.form == k.shape.form && c.runs_mode == k.runs_mode && c.shape.rtc_fill == k.shape.rtc_fill &&
        c.shape.rtc_sparse == k.shape.rtc_sparse && c.shape.weighted == k.shape.weighted) {
      return c;
    }
  }
  plan.classes.push_back(std::move(mp.cls));   // (nothing reads the plan's key after this)
  plan.classes.back().shape.threads = threads;
  return plan.classes.back();
}

// sparse flavour: members whose histogram exceeds LDS count into per-event-bin counters
int build_sparse_descs(sxmc_group* g) {
  const int n = (int)g->members.size();
  std::vector<SxSignalDesc> sparse_descs = g->h_descs;
  g->sparse_ready = false;
  g->max_bins_sparse = 0;
  // (a member with sample multiplicities: the weighted fill counts into dense histograms only, so the whole group
  // evaluates in the dense flavour -- same values at the events' bins, same norms)
  bool sparse_ok = weighted_members(g) == 0;
  for (int i = 0; i < n; i++) {
    sxmc_hist* h = g->members[i];
    if (h->total_nbins > kLdsMaxBins) {
      if (h->has_points && h->d_table) {
        make_sparse_desc(h, sparse_descs[(size_t)i]);
        // members that look up the same set of bins (the usual case: one data set, one binning) share ONE
        // filter and table, so the probes of all signals hit the same few cache lines
        for (int k = 0; k < i; k++) {
          const sxmc_hist* o = g->members[k];
          if (o->d_table && o->total_nbins == h->total_nbins && o->targets == h->targets) {
            sparse_descs[(size_t)i].sparse_filter = o->d_filter.get();
            sparse_descs[(size_t)i].sparse_table = o->d_table.get();
            sparse_descs[(size_t)i].sparse_coarse = o->d_coarse.get();
            break;
          }
        }
        g->sparse_ready = true;
      } else {
        sparse_ok = false;
      }
    }
    g->max_bins_sparse = std::max(g->max_bins_sparse, sparse_descs[(size_t)i].total_nbins);
  }
  g->sparse_ready = g->sparse_ready && sparse_ok;
  g->h_descs_sparse = sparse_descs;
  g->ec[0].descs_valid = g->ec[1].descs_valid = false;
  g->prezeroed = 0;
  if (!g->d_descs_sparse) SX_BUF(g->d_descs_sparse.alloc((size_t)std::max(n, 1)));
  if (n) SX_HIP(hipMemcpy(g->d_descs_sparse.get(), sparse_descs.data(), sizeof(SxSignalDesc) * n, hipMemcpyHostToDevice));
  return SXMC_OK;
}

// ---- threads per workgroup and LDS of a class, before its tables are laid out.  K (runs mode): workgroups per member.
void class_threads_and_lds(const sxmc_group* g, const PlanConfig& cfg, const LaunchPlan& plan, const DeviceProps& props,
                           const std::vector<MemberPlan>& plans, LaunchClass& c, std::vector<int>& K, Blocked& blocked) {
  c.max_bins = 0;
  for (int idx : c.member_idx) c.max_bins = std::max(c.max_bins, g->h_descs[(size_t)idx].total_nbins);
  c.shape.lds_bytes = c.shape.lds_hist ? ((size_t)c.max_bins + 4 + 64) * 4 : 64;
  if (is_ordered(c) && c.shape.lds_hist) {   // (replicas: class_lds_layout)
    c.shape.lds_bytes = sxplan::ordered_lds_bytes(sxplan::ordered_rstride_plain(c.max_bins), 1, 0);
  }
  c.shape.sparse_runs = 0;
  c.shape.sparse_lds_bytes = 0;
  if (c.runs_mode) {
    // every wave owns 2 x 512 words of LDS (table keys + counts) and walks its own run of consecutive granules:
    // member j gets K_j workgroups (in proportion to its granules) = K_j x waves runs.  Three workgroups of
    // 512 per CU measured best at BASELINE config 5 (2.14 ms; one of 1024: 2.29 ms; thread counts that are not
    // powers of two 2.4 ms); the kernel is bound by vector-instruction issue and HBM together, and 24 waves
    // per CU is what its registers allow.
    const int rthreads = cfg.threads > 0 ? c.shape.threads : 512;
    const size_t need = (size_t)(rthreads / 64) * 2u * ((size_t)4 << SXMC_SPARSE_SMAX_LOG2);
    std::vector<unsigned long long> sizes;
    for (int idx : c.member_idx) sizes.push_back((unsigned long long)plans[(size_t)idx].sort->lsrc.size() * 64ull);
    const int rbpc = std::min(cfg.bpc > 0 ? cfg.bpc : std::max(1, 1536 / rthreads),
                              std::max(1, (int)((size_t)props.lds_per_cu / need)));
    if (need > (size_t)props.lds_per_cu || !apportion_workgroups(sizes, props.cus * rbpc, rthreads, K)) {
      if (is_ordered(c) && !plan.order_blocked) {   // the ordered layout needs the runs: plan again without it
        blocked = Blocked::order;
        return;
      }
      c.runs_mode = false;   // (more such members than workgroups: the table stays in sorted order)
    } else {
      c.shape.threads = rthreads;
      c.shape.sparse_lds_bytes = need;
    }
  }
  if (!c.shape.lds_hist && g->sparse_ready && !c.runs_mode) {
    int cshift = 32;
    for (int idx : c.member_idx) cshift = std::min(cshift, g->members[idx]->coarse_shift);
    c.shape.lds_bytes = ((size_t)4 + ((size_t)1 << (32 - cshift - 5))) * 4;   // header + largest coarse filter
    // a filter of more than half the LDS leaves room for one workgroup per CU: make it a full one
    if (cfg.threads <= 0 && c.shape.lds_bytes * 2 > (size_t)props.lds_per_cu) c.shape.threads = 1024;
  }
  if (cfg.threads <= 0 && cfg.bpc <= 0 && c.shape.lds_hist && !is_bucketed(c) && !c.runs_mode) {
    // A SHORT launch with its histograms in LDS (BASELINE config 2: 80 MB, ~10 units per lane): the launch's fixed
    // cost is most of it, and a large part of that is the flush -- every workgroup sends its private histogram
    // to HBM with memory-side atomics.  ONE workgroup of 1024 per CU instead of two of 512 keeps the lanes and
    // halves the histograms to flush: config 2, same box, 17.6 us against 21.0 (35 700 against 33 200 evals/s;
    // 768 x 1: 18.0, 512 x 1: 21.5, 256 x 4: 27.5, 1024 x 2: 19.6; profiles/r03_c2_sweep_policy_x_shape.log).
    double bytes = 0;
    for (int idx : c.member_idx) bytes += (double)g->h_descs[(size_t)idx].nvec * SXMC_VEC * 4.0 * std::max(1, c.shape.nslot);
    if (bytes < 2.0e8) {
      c.shape.threads = 1024;
    }
  }
}

// ---- the tables of a class's members, now that the shape is known (pre-binned column, bucketed copy, codes), and their
// descriptors as the fill reads them
int class_tables(const sxmc_group* g, const PlanConfig& cfg, LaunchPlan& plan, const std::vector<MemberPlan>& plans,
                 const std::vector<int>& K, LaunchClass& c, std::vector<SxSignalDesc>& descs, Blocked& blocked) {
  const bool boxed = is_boxed(c);
  unsigned long long prefix = 0;
  for (size_t q = 0; q < c.member_idx.size(); q++) {
    const int idx = c.member_idx[q];
    SxSignalDesc d = plans[(size_t)idx].desc;
    sxmc_hist* h = g->members[idx];
    if (const int width = sx_form_pre_bytes(c.shape.form)) {
      SampleStore& st = *h->store;
      std::lock_guard<std::mutex> lock(st.pre_mutex);
      void* pre = st.find_pre(c.pre_mask, width);
      if (!pre) {
        const size_t npad = h->nvec * SXMC_VEC;
        DeviceBuffer<void> column;
        SX_BUF(column.alloc(std::max<size_t>(npad * (size_t)width, 16)));
        pre = column.get();
        st.pre.push_back({c.pre_mask, width, std::move(column)});
        SX_HIP(sx_launch_prebin(g->d_descs.get() + idx, npad, c.pre_mask, width, pre, nullptr));
        SX_HIP(hipDeviceSynchronize());
      }
      d.pre = pre;
    }
    if (c.shape.weighted) d.pre = h->mult->get();   // (the rows' multiplicities, padded with 0 to the pitch)
    if (is_bucketed(c)) {
      const int runs = c.runs_mode ? std::max(1, K[q]) * (c.shape.threads / 64) : 1;
      const SampleStore::Bucketed* bk = nullptr;
      int rc = get_bucketed(h, plans[(size_t)idx].sort, plans[(size_t)idx].fields, runs, &bk);
      if (rc) return rc;
      d.cols = bk->d_cols.get();
      d.col_pitch = bk->pitch;
      d.nsamples = bk->ngranules * 256;
      d.nvec = bk->ngranules * 64;
      d.pre = bk->d_gpre.get();
      d.edges = bk->d_gedge.get();
      d.boxes = bk->d_gbox.get();
      if (boxed) {   // (launch-wide: the largest of the members' mean extents)
        c.box_dx = std::max(c.box_dx, (float)bk->box_dx);
        c.box_dt = std::max(c.box_dt, (float)bk->box_dt);
      }
      plan.member_bucket[(size_t)idx] = bk;
      // CODES: ordered table, histogram in LDS, 2 to 4 streamed fields, every systematic on them affine (one
      // coefficient) -- the conditions fill_ordered_body's kCodes states at compile time
      // (Histograms beyond LDS, counted at the event bins over run-walked tables -- BASELINE config 5 -- were given
      // codes too and measured: bit-identical, and SLOWER, 4.0 ms against 2.1-2.6.  With 200 bins per written
      // observable a code step is 1/220 of a bin, 0.8 % of the samples are ambiguous and 87 % of the 256-sample
      // units hold one; the fix-up then runs almost everywhere.  Codes pay where bins are coarse against 2^-16 of
      // the window: not offered there.)
      bool affine = is_ordered(c) && c.shape.lds_hist && c.shape.nobs >= 1 && (boxed || c.shape.nslot - 1 >= 2) &&
                    c.shape.nslot - 1 <= SXMC_MAX_QSLOTS && !c.runs_mode && codes_enabled(cfg);
      for (unsigned w : c.prog) affine = affine && ((int)((w >> 4) & 15u) == c.shape.nslot - 1 || ((w >> 12) & 15u) == 0u);
      if (affine) {
        rc = get_bucket_codes(h, bk, d);
        if (rc) return rc;
        if (bk->d_qcol) {
          d.qcol = bk->d_qcol.get();
          for (int m = 0; m < bk->nq; m++) {
            d.qbase[m] = bk->qbase[m];
            d.qstep[m] = bk->qstep[m];
          }
          c.codes = true;
        }
      }
      if (boxed && !d.qcol) {   // (no table of codes -- too many ambiguous rows, rows outside the window, no memory: the
                                //  boxed form has no float stream of its own.  Planned again without it.)
        blocked = Blocked::box;
        return SXMC_OK;
      }
    }
    d.vec_start = prefix;
    prefix += d.nvec;
    d.step_gate = g->d_ticket.get() + sxstep::kGate;    // (read by the measurement build's gated fill only)
    descs.push_back(d);
  }
  c.total_vec = prefix;
  return SXMC_OK;
}

// Over codes, where nothing was asked for: TWO workgroups of 512 lanes per CU, each with half the replicas of the
// LDS histogram.  One of 768 or 1024 with all four replicas is as fast alone (config 3, alternating on one box:
// 81.0-81.6 us against 81.3-81.4 and 79.6-82.8), but with other chains' launches in flight -- the fake experiments
// of an ensemble -- two workgroups per CU let one launch's tail run under the next one's start: 13 280 chain-steps/s
// against 12 430 and 12 840 (profiles/r04b_codes_shapes_ab.log).  A histogram too large for two workgroups' LDS:
// one of 768.  sxmc_group_optimize times these shapes on the box it runs on.
// Sets the class's threads; returns its workgroups per CU, or 0 where the shape is not this function's to choose.
int class_codes_shape(const PlanConfig& cfg, const DeviceProps& props, LaunchClass& c) {
  if (!(c.codes && cfg.threads <= 0 && cfg.bpc <= 0)) return 0;
  const size_t one = std::max(c.shape.lds_bytes, sxplan::ordered_lds_bytes(sxplan::ordered_rstride_plain(c.max_bins), 1, 0)) +
                     ordered_queue_bytes(kMinQueueLog);
  bool codes_two = 2 * (one + 2048) <= (size_t)props.lds_per_cu && c.shape.nobs == 1;   // (+ the padded form's guard rows)
  c.shape.threads = codes_two ? 512 : 768;
  // (boxed form: one workgroup of 1024 lanes.  Config 3, one box, alternating: 64.6-66.4 us against 68.3 for 768 x 1
  // and 73.0-73.3 for 512 x 2 -- profiles/r05_boxed_ab.log)
  if (is_boxed(c)) {
    static const int forced = [] {   // (SXMC_BOX_LANES, measurement build: 512 = two workgroups of 512 per CU, 768, 1024)
      const char* e = measure_env("SXMC_BOX_LANES");
      return e ? std::atoi(e) : 0;
    }();
    codes_two = forced == 512 && codes_two;
    c.shape.threads = forced == 512 ? 512 : forced == 768 ? 768 : 1024;
  }
  return codes_two ? 2 : 1;
}

// Waves per CU.  The fill is a stream: HBM delivers most with about 32 KiB of loads in flight per CU,
// which is 512 lanes with one unit (3-4 columns x 16 bytes) each; more waves only queue up (measured
// -8 % at BASELINE config 3).  Members whose per-sample arithmetic is long (a run-time decoded program
// of two or more systematics, the shape-agnostic kernel) or that probe L2 per sample (histograms
// beyond LDS) need the second set of waves to hide it.  codes_bpc: class_codes_shape's answer.
int class_waves_per_cu(const sxmc_group* g, const PlanConfig& cfg, const DeviceProps& props, LaunchClass& c, int codes_bpc) {
  int cls_nsyst = 0;
  for (int idx : c.member_idx) cls_nsyst = std::max(cls_nsyst, g->h_descs[(size_t)idx].nsyst);
  const bool ordered = is_ordered(c);
  const double stream_bytes = (double)c.total_vec * SXMC_VEC * 4.0 * std::max(1, c.shape.nslot - (ordered ? 1 : 0));
  c.light = c.shape.lds_hist && (c.shape.nobs > 0 || ordered) &&
            (c.shape.static_prog >= 0 || c.shape.rtc_fill || cls_nsyst <= 1) &&
            stream_bytes >= 2.0e8;  // (short launches are ramp-bound: they take all the waves)
  int bpc = cfg.bpc > 0 ? cfg.bpc : codes_bpc ? codes_bpc : std::max(1, (c.light ? 512 : 1024) / c.shape.threads);
  const size_t lds_need = std::max(c.shape.lds_bytes, c.shape.sparse_lds_bytes);
  const int lds_limit = std::max(1, (int)((size_t)props.lds_per_cu / std::max<size_t>(lds_need, 1)));
  return std::min(bpc, lds_limit);
}

// The LDS of an ordered or boxed class with its histograms in LDS: replicas, padded or plain form, queues
// (sxplan::ordered_lds_layout) in the workgroup's share of the CU's LDS.
void class_lds_layout(const PlanConfig& cfg, const DeviceProps& props, LaunchClass& c, const std::vector<SxSignalDesc>& descs,
                      int bpc, Blocked& blocked) {
  c.shape.lds_layout = 0;
  if (!(is_ordered(c) && c.shape.lds_hist)) return;
  // (SXMC_LDS_RESERVE, measurement build: bytes of the CU's LDS the fill leaves to other kernels' workgroups)
  static const size_t lds_reserve = [] {
    const char* e = measure_env("SXMC_LDS_RESERVE");
    return e ? (size_t)std::max(0, std::atoi(e)) : (size_t)0;
  }();
  // (SXMC_ORDERED_REPLICAS_LOG2, measurement: fewer replicas leave LDS for a second workgroup per CU -- of another
  // chain's launch, say)
  static const unsigned rlog_max = [] {
    const char* e = measure_env("SXMC_ORDERED_REPLICAS_LOG2");
    return e ? (unsigned)std::min(std::max(std::atoi(e), 0), 2) : 2u;
  }();
  sxplan::OrderedLdsIn in;
  in.max_bins = c.max_bins;
  in.codes = c.codes;
  in.share = ((size_t)props.lds_per_cu - lds_reserve) / (size_t)std::max(1, bpc) - (fused_step_requested(cfg) ? 16 * 1024 : 0);
  in.rlog_max = rlog_max;
  in.queue_cap = cfg.queue_log;
  // the padded form of the histogram where every member qualifies (one observable binned per sample, the
  // outermost dimension) and it fits with room for the smallest queue; then the queues of ambiguous rows, in
  // what the replicas leave of the workgroup's share
  if (c.codes && c.shape.nobs == 1) in.padded_rstride = sxplan::padded_rstride_of(descs, is_boxed(c));
  // (lds.fits is deliberately not consulted: a layout beyond the share was never refused here, and refusing it now
  // would change which plans exist)
  const sxplan::OrderedLds lds = sxplan::ordered_lds_layout(in);
  c.shape.lds_layout = lds.word;
  c.shape.lds_bytes = lds.bytes;
  if (c.codes) {
    c.padded_rstride = lds.padded ? in.padded_rstride : 0;
    if (!lds.qlog) c.codes = false;   // (no room for queues: the kernel streams the float columns)
  }
  // (the boxed form exists only over codes, in the padded form with queues)
  if (is_boxed(c) && (!in.codes || !lds.qlog || !lds.padded)) blocked = Blocked::box;
}

// The class's descriptors on the device, in both flavours.
int class_upload_descs(const sxmc_group* g, const LaunchPlan& plan, LaunchClass& c, const std::vector<SxSignalDesc>& descs) {
  SX_HIP(upload(descs, c.d_descs));
  if (!(g->sparse_ready && !c.shape.lds_hist)) return SXMC_OK;
  std::vector<SxSignalDesc> sd = descs;
  for (size_t q = 0; q < sd.size(); q++) {
    sxmc_hist* h = g->members[c.member_idx[q]];
    const SxSignalDesc& shared = g->h_descs_sparse[(size_t)c.member_idx[q]];
    make_sparse_desc(h, sd[q]);
    sd[q].sparse_filter = shared.sparse_filter;  // shared tables
    sd[q].sparse_table = shared.sparse_table;
    sd[q].sparse_coarse = shared.sparse_coarse;
    if (c.runs_mode) {
      // members that look up the same set of bins share ONE set of bucket tables (one data set, one binning)
      const sxmc_hist* owner = h;
      for (size_t k = 0; k < q; k++) {
        const sxmc_hist* o = g->members[c.member_idx[k]];
        if (o->btab_valid && o->btab_mask == h->btab_mask && o->total_nbins == h->total_nbins &&
            o->targets == h->targets) {
          owner = o;
          break;
        }
      }
      sd[q].sparse_dir = owner->d_bdir.get();
      sd[q].sparse_tkeys = owner->d_btkeys.get();
      sd[q].sparse_tslot = owner->d_btslot.get();
      sd[q].pre = plan.member_bucket[(size_t)c.member_idx[q]]->d_gkp.get();   // {bucket key, bin offset} per granule
    }
  }
  SX_HIP(upload(sd, c.d_descs_sparse));
  return SXMC_OK;
}

// Who reads which units of the class's members.
int class_partition(const PlanConfig& cfg, LaunchClass& c, const std::vector<SxSignalDesc>& descs, const std::vector<int>& K) {
  if (c.shape.grid <= 0) return SXMC_OK;
  std::vector<SxSegment> segs;
  std::vector<unsigned> blk_off;
  std::vector<unsigned long long> nvec;
  for (const SxSignalDesc& d : descs) nvec.push_back(d.nvec);
  if (c.runs_mode) {
    sxplan::interleaved_segments(nvec, K, c.shape.threads, c.shape.grid, segs, blk_off);
    c.partition = 2;
  } else {
    // Bucketed tables are sorted by bin, so a member's workgroups can work as TEAMS over contiguous parts of it
    // (sxplan::interleaved_segments): a workgroup of a team of 7 sees a third of the histogram's bins, and the
    // flush -- one memory-side atomic per non-zero bin of every workgroup, 1.3 M per launch at config 3 -- sends
    // a third of the atomics, against a coarser interleaving of the stream.  Which wins depends on the BOX
    // (profiles/r03_c3_teams_sweep.log: 3 teams 129.4 us against 133.4-134.4 on one,
    // 128.4 against 124.9 on another, each consistently over alternating runs), so the default is one team and
    // sxmc_group_optimize tries three on the box it runs on (SXMC_PART_GROUPS forces a count for A/B runs).
    static const int forced_groups = [] {
      const char* e = measure_env("SXMC_PART_GROUPS");
      return e ? std::atoi(e) : 0;
    }();
    // (the boxed form, where nothing was asked for: 20 teams -- a workgroup then sees a twentieth of the sorted order,
    // its bucket or two, and flushes as few bins.  One box, alternating, two rounds (profiles/r05_boxed_teams_ab.log):
    // fill 63.4-63.5 us and step 77.9 against 65.0-65.1 and 79.9-80.0 for one team; 3-10 teams in between.)
    const bool bucketed = is_bucketed(c);
    const int groups = (bucketed && c.shape.lds_hist)
                           ? (forced_groups > 0 ? forced_groups : cfg.teams > 0 ? cfg.teams : is_boxed(c) ? 20 : 1) : 1;
    c.teams = groups;
    sxplan::build_partition(nvec, c.shape.grid, c.shape.threads, cfg.partition, segs, blk_off, c.partition,
                            bucketed ? 64 : 1, groups);
  }
  SX_HIP(upload(segs, c.d_segs, 1));
  SX_HIP(upload(blk_off, c.d_blk_off));
  return SXMC_OK;
}

// One class from its members' plans to a launch: shape, tables, LDS, grid, descriptors, partition.
int plan_class(const sxmc_group* g, const PlanConfig& cfg, LaunchPlan& plan, const DeviceProps& props,
               const std::vector<MemberPlan>& plans, LaunchClass& c, Blocked& blocked) {
  std::vector<int> K;   // runs mode: workgroups per member
  class_threads_and_lds(g, cfg, plan, props, plans, c, K, blocked);
  if (blocked != Blocked::none) return SXMC_OK;
  std::vector<SxSignalDesc> descs;
  int rc = class_tables(g, cfg, plan, plans, K, c, descs, blocked);
  if (rc || blocked != Blocked::none) return rc;
  const int codes_bpc = class_codes_shape(cfg, props, c);   // (sets shape.threads, which the next line reads)
  const int bpc = class_waves_per_cu(g, cfg, props, c, codes_bpc);
  class_lds_layout(cfg, props, c, descs, bpc, blocked);
  if (blocked != Blocked::none) return SXMC_OK;
  const unsigned long long want = (c.total_vec + c.shape.threads - 1) / c.shape.threads;  // >= 1 unit per lane
  const unsigned long long grid = std::max<unsigned long long>(1, std::min((unsigned long long)props.cus * bpc, want));
  c.shape.grid = c.total_vec ? (int)grid : 0;
  if (c.runs_mode) {
    int used = 0;
    for (int k : K) used += k;
    c.shape.grid = used;
    c.shape.sparse_runs = 1;
  }
  rc = class_upload_descs(g, plan, c, descs);
  return rc ? rc : class_partition(cfg, c, descs, K);
}

// What both forms of the plan share, once per rebuild: the members' descriptors in member order, in both flavours,
// and what the group keeps about them.
int plan_shared_descs(sxmc_group* g) {
  // Descriptors may still be read by kernels in flight on another stream: rebuilds are rare
  // (bindings change only during setup), so a device-wide sync is the simple safe choice.
  SX_HIP(hipDeviceSynchronize());
  const int n = (int)g->members.size();
  g->h_descs.assign((size_t)n, SxSignalDesc{});
  g->max_bins = 0;
  g->max_points = 0;
  g->same_points = n > 0;
  for (int i = 0; i < n; i++) {
    const sxmc_hist* h = g->members[i];
    fill_desc(h, g->h_descs[i]);
    g->max_bins = std::max(g->max_bins, h->total_nbins);
    g->max_points = std::max<unsigned long long>(g->max_points, g->h_descs[i].npoints);
    if (!h->has_points || h->npoints != g->members[0]->npoints) g->same_points = false;
  }
  if (!g->d_descs) SX_BUF(g->d_descs.alloc((size_t)std::max(n, 1)));
  if (n) SX_HIP(hipMemcpy(g->d_descs.get(), g->h_descs.data(), sizeof(SxSignalDesc) * n, hipMemcpyHostToDevice));
  return build_sparse_descs(g);
}

// One pass over a plan, from the members' forms to the classes' launches.  `blocked`: a step found the ordered or the
// boxed form cannot be laid out; what the pass has allocated is freed by the next one's start.
int plan_pass(sxmc_group* g, const PlanConfig& cfg, const DeviceProps& props, LaunchPlan& plan, Blocked& blocked) {
  plan.clear();
  int threads = cfg.threads > 0 ? cfg.threads : 512;
  if (threads < 64 || threads > 1024 || threads % 64) threads = 512;
  const int n = (int)g->members.size();
  std::vector<MemberPlan> plans((size_t)n);
  plan.member_bucket.assign((size_t)n, nullptr);
  for (int i = 0; i < n; i++) {
    int rc = plan_member(g, cfg, plan, props, i, plans[(size_t)i]);
    if (rc) return rc;
    find_class(plan, plans[(size_t)i], threads).member_idx.push_back(i);
  }
  for (LaunchClass& c : plan.classes) {
    int rc = plan_class(g, cfg, plan, props, plans, c, blocked);
    if (rc || blocked != Blocked::none) return rc;
  }
  return SXMC_OK;
}

// The plan of `cfg`: passes until no step is blocked (at most three: each of the plan's two flags is set once).
int plan_form(sxmc_group* g, const PlanConfig& cfg, const DeviceProps& props, LaunchPlan& plan) {
  for (;;) {
    Blocked blocked = Blocked::none;
    int rc = plan_pass(g, cfg, props, plan, blocked);
    if (rc || blocked == Blocked::none) return rc;
    (blocked == Blocked::order ? plan.order_blocked : plan.box_blocked) = true;
  }
}

inline bool any_boxed(const LaunchPlan& plan) { return std::any_of(plan.classes.begin(), plan.classes.end(), is_boxed); }

// BOXED plans, plan_cfg.box < 0 (the default): the boxed form is fast only while few boxes straddle an edge, which depends on
// the parameters of the evaluation.  The same members are therefore planned a second time in the ORDERED form (g->ordered:
// the same passes with box = 0 over the same descriptors), group_fill launches the plan `fill_form` names, and the host
// moves that between flushes of a walk (sxmc_group_adapt_fill_form).  Until it is asked to, the ordered form runs: a caller
// that never asks gets round 4's kernel.  No ordered plan (the form does not apply): the plan is built again without boxes.
int group_rebuild(sxmc_group* g) {
  TraceRange trace("sxmc: launch plan (tables, partitions, kernels)");
  DeviceProps props;
  int rc = get_props(props);
  if (rc) return rc;
  rc = plan_shared_descs(g);
  if (rc) return rc;
  bool two = false;
  for (;;) {
    rc = plan_form(g, g->plan_cfg, props, g->plan);
    if (rc) return rc;
    two = g->plan_cfg.box < 0 && any_boxed(g->plan);
    if (!two) break;
    PlanConfig ordered_cfg = g->plan_cfg;
    ordered_cfg.box = 0;
    rc = plan_form(g, ordered_cfg, props, g->ordered);
    if (rc) return rc;
    if (!g->ordered.classes.empty() && !any_boxed(g->ordered)) break;
    g->plan.box_blocked = true;
  }
  if (!two) g->ordered.clear();   // (what has_two_forms asks)
  for (LaunchClass& c : g->plan.classes) c.dual = two && is_boxed(c);
  g->fill_form = two && g->fill_form != 1 ? 2 : 1;   // (one form: the plan's own launches; a form of 1 survives a replan)
  const size_t n = g->members.size();
  g->seen.resize(n);
  g->seen_points.resize(n);
  for (size_t i = 0; i < n; i++) {
    g->seen[i] = g->members[i]->version;
    g->seen_points[i] = g->members[i]->points_version;
  }
  g->plan_cfg_seen = g->plan_cfg;
  g->plan_generation++;
  g->built = true;
  return SXMC_OK;
}

// New evaluation points of the same size class (same buffers, sxmc_hist_set_eval_points) change two fields of
// the members' descriptors and nothing else: they are patched and re-uploaded, with no device-wide
// synchronisation and no re-planning, so a fake experiment's set-up does not stall the other chains on the GPU.
int group_update_points(sxmc_group* g) {
  const int n = (int)g->members.size();
  g->max_points = 0;
  g->same_points = n > 0;
  for (int i = 0; i < n; i++) {
    sxmc_hist* h = g->members[i];
    const unsigned long long np = h->has_points ? h->npoints : 0;
    for (std::vector<SxSignalDesc>* set : {&g->h_descs, &g->h_descs_sparse}) {
      (*set)[(size_t)i].read_bins = h->has_points ? h->d_read_bins.get() : nullptr;
      (*set)[(size_t)i].npoints = np;
    }
    g->max_points = std::max(g->max_points, np);
    if (!h->has_points || h->npoints != g->members[0]->npoints) g->same_points = false;
    g->seen_points[(size_t)i] = h->points_version;
  }
  if (n) {
    SX_HIP(hipMemcpy(g->d_descs.get(), g->h_descs.data(), sizeof(SxSignalDesc) * n, hipMemcpyHostToDevice));
    SX_HIP(hipMemcpy(g->d_descs_sparse.get(), g->h_descs_sparse.data(), sizeof(SxSignalDesc) * n, hipMemcpyHostToDevice));
  }
  g->ec[0].descs_valid = g->ec[1].descs_valid = false;
  return SXMC_OK;
}

int group_refresh(sxmc_group* g) {
  bool stale = !g->built || !(g->plan_cfg_seen == g->plan_cfg);
  bool points = false;
  for (size_t i = 0; !stale && i < g->members.size(); i++) {
    if (g->seen[i] != g->members[i]->version) stale = true;
    if (g->seen_points[i] != g->members[i]->points_version) points = true;
  }
  if ((stale || points) && t_capturing) {
    return fail(SXMC_ERR_STATE, "the group's launch plan is out of date: evaluate once before recording a graph");
  }
  if (stale) return group_rebuild(g);
  return points ? group_update_points(g) : SXMC_OK;
}

int group_check_bound(sxmc_group* g, bool need_pdf) {
  for (sxmc_hist* h : g->members) {
    if (!h->norm) return fail(SXMC_ERR_STATE, "evaluation before SetNormalizationBuffer");
    if (!h->systs.empty() && !h->params) return fail(SXMC_ERR_STATE, "evaluation before SetParameterBuffer");
    if (need_pdf && h->has_points && !h->pdf) return fail(SXMC_ERR_STATE, "evaluation before SetPDFValueBuffer");
  }
  return SXMC_OK;
}

// Event classes of one descriptor flavour, built on the host from the members' event-bin tables:
// events with the same bin (counter slot) in every member contribute the same term to the event sum,
// so the sum runs over the distinct tuples, each weighted by its multiplicity.  Tables are rebuilt when
// evaluation points change, the descriptor copies whenever the group is rebuilt.
int ensure_event_classes(sxmc_group* g, bool sparse) {
  sxmc_group::EventClasses& ec = g->ec[sparse ? 1 : 0];
  const size_t S = g->members.size();
  bool tables_ok = ec.tables_valid && ec.seen_points.size() == S;
  for (size_t j = 0; tables_ok && j < S; j++) tables_ok = ec.seen_points[j] == g->members[j]->points_version;
  if (tables_ok && ec.descs_valid) return SXMC_OK;
  if (t_capturing) {
    return fail(SXMC_ERR_STATE, "the event classes are out of date: evaluate once before recording a graph");
  }
  // (the caller is done with the group's previous evaluations; buffers are re-used, so nothing stalls the device)
  const std::vector<SxSignalDesc>& flavour = sparse ? g->h_descs_sparse : g->h_descs;
  if (!tables_ok) {
    const size_t E = g->members[0]->npoints;
    // the table each member's descriptor of this flavour reads
    std::vector<const std::vector<int>*> arr(S);
    for (size_t j = 0; j < S; j++) {
      const sxmc_hist* h = g->members[j];
      const bool slots = sparse && flavour[j].read_bins == h->d_read_slot.get() && h->d_read_slot;
      arr[j] = slots ? &h->h_read_slot : &h->h_read_bins;
      if (arr[j]->size() != E) return fail(SXMC_ERR_STATE, "event-bin table of a member is missing");
    }
    sxplan::EventClasses cls;   // distinct tuples of event bins + multiplicities (sxmc_plan.h)
    sxplan::event_classes(arr, E, cls);
    const size_t K = cls.K;
    const std::vector<int>& tables = cls.tables;
    const std::vector<unsigned>& weight = cls.weight;
    if (tables.size() > ec.d_rb.capacity()) SX_BUF(ec.d_rb.grow(tables.size() + tables.size() / 4));
    if (std::max<size_t>(K, 1) > ec.d_weight.capacity()) SX_BUF(ec.d_weight.grow(K + K / 4 + 16));
    SX_HIP(hipMemcpy(ec.d_rb.get(), tables.data(), sizeof(int) * tables.size(), hipMemcpyHostToDevice));
    if (K) SX_HIP(hipMemcpy(ec.d_weight.get(), weight.data(), sizeof(unsigned) * K, hipMemcpyHostToDevice));
    if (!g->event_weights.empty()) {
      // real event weights (sxmc_group_set_event_weights: it drops these tables, as new points do): the classes' sums
      if (g->event_weights.size() != E) {
        return fail(SXMC_ERR_STATE, "the group's event weights are not one per evaluation point of its members");
      }
      std::vector<double> W;
      sxplan::class_weights(arr, E, cls, g->event_weights.data(), W);
      if (std::max<size_t>(K, 1) > ec.d_real_weight.capacity()) SX_BUF(ec.d_real_weight.grow(K + K / 4 + 16));
      if (K) SX_HIP(hipMemcpy(ec.d_real_weight.get(), W.data(), sizeof(double) * K, hipMemcpyHostToDevice));
    }
    ec.K = K;
    ec.seen_points.resize(S);
    for (size_t j = 0; j < S; j++) ec.seen_points[j] = g->members[j]->points_version;
    ec.tables_valid = true;
    ec.descs_valid = false;
  }
  std::vector<SxSignalDesc> descs = flavour;
  for (size_t j = 0; j < S; j++) {
    descs[j].read_bins = ec.d_rb.get() + j * ec.K;
    descs[j].npoints = ec.K;
    descs[j].pdf_out = nullptr;
  }
  if (!ec.d_descs) SX_BUF(ec.d_descs.alloc(std::max<size_t>(S, 1)));
  SX_HIP(hipMemcpy(ec.d_descs.get(), descs.data(), sizeof(SxSignalDesc) * S, hipMemcpyHostToDevice));
  // (the by-value form of the same descriptors: a kernel argument, so a recorded step end holds the copy it was recorded
  // with -- like the row count and the weights beside it; this function refuses to rebuild any of them under a recording)
  ec.has_table = sx_step_end_table_fill(ec.table, descs.data(), S);
  ec.descs_valid = true;
  return SXMC_OK;
}

// What precedes a group's fill launches: the zeroing (unless the last step end already cleared for this
// evaluation) and the bookkeeping of who cleared what.
int group_prepare_fill(sxmc_group* g, hipStream_t s, bool sparse) {
  // Recorded launches do not run now, so what a recording "pre-zeroed" is not zero yet: the first
  // evaluation of every recording zeroes explicitly, and sxmc_graph_end_capture drops the flag.
  bool first_in_recording = false;
  if (t_capturing && g->capture_epoch != t_capture_epoch) {
    g->capture_epoch = t_capture_epoch;
    t_capture_groups.push_back(g);
    first_in_recording = true;
  }
  bool skip_zero = g->prezeroed == (sparse ? 2 : 1) && !first_in_recording;
  for (sxmc_hist* h : g->members) {  // (an evaluator may also be evaluated alone or through another group)
    skip_zero = skip_zero && h->cleared_by == g;
    h->cleared_by = nullptr;
  }
  g->prezeroed = 0;
  g->last_sparse = sparse;
  if (!skip_zero) {
    SX_HIP(sx_launch_zero(sparse ? g->d_descs_sparse.get() : g->d_descs.get(), (int)g->members.size(),
                          sparse ? g->max_bins_sparse : g->max_bins, g->d_ticket.get(), s));
  }
  for (size_t i = 0; i < g->members.size(); i++) {
    g->members[i]->bins_valid = g->members[i]->total_nbins > kLdsMaxBins ? !sparse : true;
  }
  return SXMC_OK;
}

int group_fill(sxmc_group* g, hipStream_t s, bool sparse) {
  TraceRange trace("sxmc: fill (EvalHist of all signals)");
  sparse = sparse && g->sparse_ready && g->cfg_sparse;
  int rc = group_prepare_fill(g, s, sparse);
  if (rc) return rc;
  // (a plan with two forms: the launches of the one fill_form names -- sxmc_group_adapt_fill_form)
  for (LaunchClass& c : active_plan(g).classes) {
    // profiled launches (sxmc_group_profile) carry two events stamped with the dispatch's own begin and end
    const bool rec = g->prof && !t_capturing && g->prof_n < (int)g->ev0.size() && c.shape.grid > 0;
    c.shape.ev_start = rec ? (void*)g->ev0[g->prof_n] : nullptr;
    c.shape.ev_stop = rec ? (void*)g->ev1[g->prof_n] : nullptr;
    c.shape.debug_mode = g->debug_mode;
    if (sparse && c.d_descs_sparse && c.shape.sparse_runs) {
      SX_HIP(sx_launch_fill_sparse_runs(c.shape, c.d_descs_sparse.get(), c.d_segs.get(), c.d_blk_off.get(), s));
    } else {
      SX_HIP(sx_launch_fill(c.shape, (sparse && c.d_descs_sparse) ? c.d_descs_sparse.get() : c.d_descs.get(), c.d_segs.get(),
                            c.d_blk_off.get(), s));
    }
    c.shape.ev_start = c.shape.ev_stop = nullptr;
    if (rec) g->prof_n++;
  }
  return SXMC_OK;
}

}  // namespace sxhost
