// sxmc_plan.h -- the HOST PLANNERS of libsxmc_hip.so: every table the gfx950 kernels index blindly is laid out by
// one of these functions, from plain vectors into plain vectors, with no HIP call and no library state.  sxmc_launch_plan.cpp
// calls them and uploads what they return; tests/cpp/test_plan.cpp calls the same functions with randomized shapes
// under AddressSanitizer + UndefinedBehaviorSanitizer, replays the kernels' addressing against the results and
// checks that nothing is missed, counted twice or addressed out of range -- without a device.
//
//   apportion_workgroups / interleaved_segments / build_partition   who reads which units (SxSegment lists)
//   eval_point_bins        EvalHist::SetEvalPoints' loop, src/pdfz.cpp:264-301
//   build_sparse_tables    sparse counting (histograms beyond LDS): bit filters + open-addressing table
//   bucket_granules / bucket_key_offsets / bucketed_layout   bucketed copies of a sample table (layout_kernels.hip)
//   bucket_tables          per-bucket event-bin tables of fill_sparse_kernel
//   event_classes          distinct tuples of event bins, weighted by multiplicity (eval_nll_kernel)
//   columns_error          the column table of a mixed fit (sxmc_group_set_columns)
//   code_windows / ordered_lds_layout / padded_rstride_of   codes and LDS of the ordered and boxed fills
//   syst_use / choose_ordered / choose_boxed / compact_slots / prebin_columns   the form a member's table takes
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "sxmc_device_types.h"

namespace sxplan {

inline int ceil_log2(size_t x) {
  int b = 0;
  while (((size_t)1 << b) < x) b++;
  return b;
}

// ---------------------------------------------------------------------------------------------- work partition
// Cut a launch's work (units of SXMC_VEC samples) into per-workgroup segment lists.
//  interleaved: member j gets K_j workgroups (proportional to its size, sum = grid); workgroup i of
//    the member takes chunks i, i + K_j, ... of `threads` units: neighbouring workgroups read
//    neighbouring chunks at the same time and every workgroup flushes one histogram once.
//  sliced: workgroup b owns the contiguous slice [total*b/G, total*(b+1)/G) of the concatenated
//    members: perfectly balanced, used when members outnumber workgroups or are tiny.
// Largest-remainder apportionment of `grid` workgroups over members of `sizes` units: at least one per
// non-empty member and never more than the member has chunks of `threads` units.  false: they do not fit.
inline bool apportion_workgroups(const std::vector<unsigned long long>& sizes, int grid, int threads,
                                 std::vector<int>& K) {
  K.assign(sizes.size(), 0);
  unsigned long long total = 0;
  for (unsigned long long n : sizes) total += n;
  if (total == 0) return true;
  int used = 0;
  std::vector<std::pair<double, int>> frac;
  for (size_t j = 0; j < sizes.size(); j++) {
    if (!sizes[j]) continue;
    const double share = (double)grid * (double)sizes[j] / (double)total;
    const unsigned long long chunks = (sizes[j] + threads - 1) / threads;
    K[j] = (int)std::min<unsigned long long>(chunks, std::max<unsigned long long>(1, (unsigned long long)share));
    used += K[j];
    frac.push_back({share - std::floor(share), (int)j});
  }
  std::sort(frac.begin(), frac.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
  for (size_t i = 0; used < grid && !frac.empty() && i < 4 * frac.size(); i++) {
    const int j = frac[i % frac.size()].second;
    const unsigned long long chunks = (sizes[(size_t)j] + threads - 1) / threads;
    if ((unsigned long long)K[(size_t)j] < chunks) {
      K[(size_t)j]++;
      used++;
    }
  }
  return used <= grid;
}

// Workgroup i of member j takes chunks i, i + K_j, ... of `threads` units of the member (nvec[j] units).
// groups > 1 (tables whose rows are SORTED by bin -- bucketed copies): the member's workgroups are split into `groups`
// teams, team t takes a contiguous part of the member (sized by its share of the workgroups, cut at multiples of
// `threads` units) and interleaves inside it.  Neighbouring workgroups of a team still read neighbouring chunks at
// the same time (DRAM locality), but a workgroup now sees only its team's part of the sorted order, i.e. a fraction
// of the histogram's bins -- and the flush sends one memory-side atomic per NON-ZERO bin of every workgroup.
inline void interleaved_segments(const std::vector<unsigned long long>& nvec, const std::vector<int>& K, int threads,
                                 int grid, std::vector<SxSegment>& segs, std::vector<unsigned>& blk_off,
                                 int groups = 1) {
  segs.clear();
  blk_off.assign(1, 0u);
  for (size_t j = 0; j < nvec.size(); j++) {
    const int Kj = K[j];
    if (Kj <= 0) continue;
    const int G = std::max(1, std::min(groups, Kj));
    const unsigned long long chunks = (nvec[j] + (unsigned long long)threads - 1) / (unsigned long long)threads;
    int wg0 = 0;
    unsigned long long chunk0 = 0;
    for (int t = 0; t < G; t++) {
      const int wg1 = (int)((long long)Kj * (t + 1) / G);                     // workgroups [wg0, wg1) form team t
      const unsigned long long chunk1 = t + 1 == G ? chunks : chunks * (unsigned long long)wg1 / (unsigned long long)Kj;
      const int Kt = wg1 - wg0;
      for (int i = 0; i < Kt; i++) {
        SxSegment sg{};
        sg.sig = (int)j;
        sg.v0 = (chunk0 + (unsigned long long)i) * (unsigned long long)threads;
        sg.v1 = std::min(nvec[j], chunk1 * (unsigned long long)threads);
        sg.step = (unsigned long long)Kt * (unsigned long long)threads;
        // (a team with more workgroups than chunks: the spare ones get nothing -- an empty list, not an empty segment,
        // because the kernels clamp loads to v1 - 1)
        if (sg.v0 < sg.v1) segs.push_back(sg);
        blk_off.push_back((unsigned)segs.size());
      }
      wg0 = wg1;
      chunk0 = chunk1;
    }
  }
  while ((int)blk_off.size() < grid + 1) blk_off.push_back((unsigned)segs.size());  // idle workgroups
}

// want_mode: 0 auto, 1 sliced, 2 interleaved.  mode_out: what was built.  align: slices start on multiples of
// `align` units (bucketed tables: granule boundaries; every member's unit count is then a multiple of it).
inline void build_partition(const std::vector<unsigned long long>& nvec, int grid, int threads, int want_mode,
                            std::vector<SxSegment>& segs, std::vector<unsigned>& blk_off, int& mode_out,
                            unsigned long long align = 1, int groups = 1) {
  segs.clear();
  blk_off.assign(1, 0u);
  unsigned long long total = 0;
  int nonempty = 0;
  for (unsigned long long n : nvec) {
    total += n;
    if (n) nonempty++;
  }
  bool interleave = want_mode == 2 || (want_mode == 0 && nonempty > 0 && grid >= 2 * nonempty &&
                                       total >= (unsigned long long)grid * threads * 8ull);
  if (want_mode == 2 && (nonempty == 0 || grid < nonempty)) interleave = false;
  std::vector<int> K;
  if (interleave) interleave = apportion_workgroups(nvec, grid, threads, K);  // false: more members than workgroups
  if (interleave) {
    interleaved_segments(nvec, K, threads, grid, segs, blk_off, groups);
    mode_out = 2;
    return;
  }
  for (int b = 0; b < grid; b++) {
    unsigned long long r0 = total * (unsigned long long)b / grid / align * align;
    const unsigned long long r1 = b + 1 == grid ? total : total * (unsigned long long)(b + 1) / grid / align * align;
    unsigned long long start = 0;
    for (size_t j = 0; j < nvec.size() && r0 < r1; j++) {
      const unsigned long long s0 = start, s1 = start + nvec[j];
      start = s1;
      if (s1 <= r0) continue;
      SxSegment sg{};
      sg.sig = (int)j;
      sg.v0 = r0 - s0;
      sg.v1 = std::min(r1, s1) - s0;
      sg.step = (unsigned long long)threads;
      segs.push_back(sg);
      r0 = std::min(r1, s1);
    }
    blk_off.push_back((unsigned)segs.size());
  }
  mode_out = 1;
}

// ---------------------------------------------------------------------------------------------- evaluation points
// EvalHist::SetEvalPoints (pdfz.cpp:264-301): the flat bin of every evaluation point, -1 outside the domain (NaN
// coordinates included; also an index that rounds up past the end, where the reference would read one past the end
// in eval_pdf), -2 for a point of another data set.  points: rows of D + 1 floats.
inline void eval_point_bins(const float* points, size_t n, int D, const double* lower, const double* upper,
                            const double* scale, const int* stride, int total_nbins, unsigned dataset,
                            std::vector<int>& rb) {
  const size_t row = (size_t)D + 1;
  rb.resize(n);
  for (size_t ip = 0; ip < n; ip++) {
    bool in_domain = true;
    int bin_id = 0;
    for (int k = 0; k < D; k++) {
      const double element = points[row * ip + (size_t)k];
      if (!(element >= lower[k] && element < upper[k])) {
        in_domain = false;
        break;
      }
      bin_id += (int)((element - lower[k]) * scale[k]) * stride[k];
    }
    if (in_domain && (unsigned)bin_id >= (unsigned)total_nbins) in_domain = false;
    if (points[row * ip + (size_t)D] != (float)dataset) bin_id = -2;  // pdfz.cpp:289-293
    rb[ip] = in_domain ? bin_id : -1;
  }
}

// ---------------------------------------------------------------------------------------------- sparse counting
// Sparse-counting structures of one evaluator from its event bins (once per SetEvalPoints): the sorted distinct
// event bins ("targets"; a bin's rank is its counter slot), every point's slot, a fine and a coarse bit filter
// and an open-addressing table {bin, slot} -- hashed exactly as fill_kernels.inc.h looks them up.
struct SparseTables {
  std::vector<unsigned> targets;
  std::vector<int> slot;                   // per evaluation point: counter slot, or the point's negative code
  std::vector<unsigned> coarse, filter, table;
  int cbits = 0, fbits = 0, tbits = 0;     // the kernels shift hashes right by 32 - bits
};

inline void build_sparse_tables(const std::vector<int>& rb, SparseTables& o) {
  o.targets.clear();
  for (int b : rb)
    if (b >= 0) o.targets.push_back((unsigned)b);
  std::sort(o.targets.begin(), o.targets.end());
  o.targets.erase(std::unique(o.targets.begin(), o.targets.end()), o.targets.end());
  const size_t T = o.targets.size();
  o.slot.resize(rb.size());
  for (size_t i = 0; i < rb.size(); i++) {
    o.slot[i] = rb[i] < 0 ? rb[i]
                          : (int)(std::lower_bound(o.targets.begin(), o.targets.end(), (unsigned)rb[i]) - o.targets.begin());
  }
  o.fbits = std::min(26, std::max(16, ceil_log2(64 * std::max<size_t>(T, 1))));  // <= 1.6 % false positives
  o.tbits = std::max(6, ceil_log2(2 * std::max<size_t>(T, 1)));                   // load <= 50 %
  // coarse filter: two hashes per bin, >= 8 bits per bin up to 2^20 bits (128 KiB of LDS): ~3 % false
  // positives at 1e5 event bins (one hash in 64 KiB let 19 % through, and every survivor costs L2 probes)
  o.cbits = std::min(20, std::max(10, ceil_log2(16 * std::max<size_t>(T, 1))));
  o.coarse.assign((size_t)1 << (o.cbits - 5), 0u);
  o.filter.assign((size_t)1 << (o.fbits - 5), 0u);
  o.table.assign((size_t)2 << o.tbits, 0xFFFFFFFFu);
  const unsigned mask = (1u << o.tbits) - 1u;
  for (size_t t = 0; t < T; t++) {
    const unsigned bin = o.targets[t];
    const unsigned hb = (bin * 0x9E3779B1u) >> (32 - o.fbits);
    o.filter[hb >> 5] |= 1u << (hb & 31u);
    const unsigned hc = (bin * 0xC2B2AE35u) >> (32 - o.cbits), hd = (bin * 0x27D4EB2Fu) >> (32 - o.cbits);
    o.coarse[hc >> 5] |= 1u << (hc & 31u);
    o.coarse[hd >> 5] |= 1u << (hd & 31u);
    unsigned hp = (bin * 0x85EBCA6Bu) >> (32 - o.tbits);
    while (o.table[2 * (size_t)hp] != 0xFFFFFFFFu) hp = (hp + 1u) & mask;
    o.table[2 * (size_t)hp] = bin;
    o.table[2 * (size_t)hp + 1] = (unsigned)t;
  }
}

// ---------------------------------------------------------------------------------------------- bucketed tables
// A table's rows sorted by bucket key (the mixed-radix tuple of the untouched observables' bin indices).
// first[k] = position of key k's first row in the sorted order (0xFFFFFFFF: no such row), first[outside] = where
// the rows outside the domain of an untouched observable start (they sort last and are dropped).  The kept rows are
// cut into LOGICAL GRANULES of at most 256 rows, bucket by bucket, each bucket padded to whole granules.
struct GranulePlan {
  std::vector<unsigned> present;           // bucket keys that have rows, ascending
  std::vector<unsigned> lsrc, lvalid, lwhich;   // per granule: first row in the sorted order, rows, index in `present`
  size_t kept = 0;                         // rows kept (inside the domain of every untouched observable)
  bool worth_it = false;                   // false: mostly padding -- the table stays in row order
};

inline void bucket_granules(const std::vector<unsigned>& first, unsigned outside, size_t n, GranulePlan& g) {
  g = GranulePlan();
  g.kept = first[outside] != 0xFFFFFFFFu ? first[outside] : n;
  for (unsigned k = 0; k < outside; k++)
    if (first[k] != 0xFFFFFFFFu) g.present.push_back(k);
  for (size_t i = 0; i < g.present.size(); i++) {
    const size_t lo = first[g.present[i]], hi = i + 1 < g.present.size() ? first[g.present[i + 1]] : g.kept;
    for (size_t at = lo; at < hi; at += 256) {
      g.lsrc.push_back((unsigned)at);
      g.lvalid.push_back((unsigned)std::min<size_t>(256, hi - at));
      g.lwhich.push_back((unsigned)i);
    }
  }
  g.worth_it = !((double)g.lsrc.size() * 256.0 > 1.3 * (double)g.kept + 16384.0);
  if (!g.worth_it) {
    g.lsrc.clear();
    g.lvalid.clear();
    g.lwhich.clear();
  }
}

// The constant contribution of a bucket to the flat bin index: sum over the untouched observables (mask) of
// index * stride, the index decoded from the key with the bases nbins + 1 (radix[k] = product of the bases of the
// untouched observables after k).
inline void bucket_key_offsets(const std::vector<unsigned>& present, unsigned mask, const unsigned* radix,
                               const int* nbins, const int* stride, int nobs, std::vector<unsigned>& key_pre) {
  key_pre.resize(present.size());
  for (size_t i = 0; i < present.size(); i++) {
    long long pre = 0;
    for (int k = 0; k < nobs; k++) {
      if (!((mask >> k) & 1u)) continue;
      const unsigned idx = (present[i] / radix[k]) % ((unsigned)nbins[k] + 1u);
      pre += (long long)idx * stride[k];
    }
    key_pre[i] = (unsigned)pre;
  }
}

// The PHYSICAL granule order of a bucketed copy laid out for `runs` runs: run r holds logical granules
// [r * T, (r + 1) * T), runs interleaved granule by granule (physical p = t * runs + r), so that `runs` consumers
// that each walk one run read neighbouring addresses at the same time.  runs = 1: the sorted order itself.
// Per physical granule: psrc / pvalid (what the gather kernel copies), ppre (the granule word: the bucket's bin
// offset; with pack_rows -- ordered tables, histogram in LDS, offset < 2^24 -- the row count - 1 in the top byte),
// pkp = {bucket key, granule word} for the sparse kernel.
struct BucketedLayout {
  std::vector<unsigned> psrc, pvalid, ppre, pkp;
  size_t P = 0, A = 1;   // physical granules; array length (>= 1)
};

inline void bucketed_layout(const std::vector<unsigned>& lsrc, const std::vector<unsigned>& lvalid,
                            const std::vector<unsigned>& lwhich, const std::vector<unsigned>& keys,
                            const std::vector<unsigned>& key_pre, unsigned outside, int runs, bool pack_rows,
                            BucketedLayout& o) {
  const size_t L = lsrc.size();
  const size_t T = (L + (size_t)runs - 1) / (size_t)runs;
  o.P = T * (size_t)runs;
  o.A = std::max<size_t>(o.P, 1);
  o.psrc.assign(o.A, 0u);
  o.pvalid.assign(o.A, 0u);
  o.ppre.assign(o.A, 0u);
  o.pkp.assign(2 * o.A, 0u);
  for (size_t p = 0; p < o.P; p++) {
    const size_t r = p % (size_t)runs, t = p / (size_t)runs, l = r * T + t;
    if (l < L) {
      o.psrc[p] = lsrc[l];
      o.pvalid[p] = lvalid[l];
      o.ppre[p] = key_pre[lwhich[l]];
      if (pack_rows) o.ppre[p] |= (lvalid[l] - 1u) << 24;
      o.pkp[2 * p] = keys[lwhich[l]];
    } else {  // padding granule at the end of the last runs: no samples, stays in the last bucket
      o.pkp[2 * p] = L ? keys[lwhich[L - 1]] : outside;
    }
    o.pkp[2 * p + 1] = o.ppre[p];
  }
}

// The evaluator's event bins grouped by the buckets of a sort (fill_sparse_kernel): per bucket key an
// open-addressing table keyed by the event bin's index contribution of the WRITTEN observables (flat index minus
// the bucket's offset, canonical decomposition), value = the event bin's counter slot (its rank among the sorted
// distinct event bins).  dir[2 key] = the table's offset in tkeys / tslot, dir[2 key + 1] = log2(size) | probes << 8,
// or SXMC_SPARSE_EMPTY (no event bin in the bucket) / SXMC_SPARSE_SLOW (every sample through the global table).
struct BucketTables {
  std::vector<unsigned> dir, tkeys, tslot;
};

inline void bucket_tables(unsigned nkeys, unsigned mask, const unsigned* radix, const int* nbins, const int* stride,
                          int D, const std::vector<unsigned>& targets, BucketTables& o) {
  o.dir.assign(2 * ((size_t)nkeys + 1), 0u);
  o.tkeys.clear();
  o.tslot.clear();
  for (size_t k = 0; k <= nkeys; k++) o.dir[2 * k + 1] = SXMC_SPARSE_EMPTY;
  // bucket keys with an index equal to nbins: their samples alias into other rows of the flat index
  for (unsigned key = 0; key < nkeys; key++) {
    for (int k = 0; k < D; k++) {
      if (!((mask >> k) & 1u)) continue;
      if ((key / radix[k]) % ((unsigned)nbins[k] + 1u) == (unsigned)nbins[k]) o.dir[2 * (size_t)key + 1] = SXMC_SPARSE_SLOW;
    }
  }
  std::vector<std::vector<std::pair<unsigned, unsigned>>> by_key;   // only for keys that have some
  std::vector<int> where((size_t)nkeys, -1);
  for (size_t t = 0; t < targets.size(); t++) {
    const unsigned flat = targets[t];
    unsigned key = 0, pre = 0;
    for (int k = 0; k < D; k++) {
      if (!((mask >> k) & 1u)) continue;
      const unsigned idx = (flat / (unsigned)stride[k]) % (unsigned)nbins[k];
      key += idx * radix[k];
      pre += idx * (unsigned)stride[k];
    }
    if (where[key] < 0) {
      where[key] = (int)by_key.size();
      by_key.emplace_back();
    }
    by_key[(size_t)where[key]].push_back({flat - pre, (unsigned)t});
  }
  for (unsigned key = 0; key < nkeys; key++) {
    if (where[key] < 0) continue;
    const auto& list = by_key[(size_t)where[key]];
    // cells of four keys (one 16-byte LDS read per probe); load <= 25 %, or <= 50 % for the largest buckets
    int lg = std::max(2, ceil_log2(4 * list.size()));
    if (lg > SXMC_SPARSE_SMAX_LOG2) lg = std::max(2, ceil_log2(2 * list.size()));
    if (lg > SXMC_SPARSE_SMAX_LOG2) {                                  // more event bins than a wave's slice holds
      o.dir[2 * (size_t)key + 1] = SXMC_SPARSE_SLOW;
      continue;
    }
    const size_t off = o.tkeys.size(), S = (size_t)1 << lg, cells = S / 4;
    o.tkeys.resize(off + S, 0xFFFFFFFFu);
    o.tslot.resize(off + S, 0u);
    unsigned probes = 1;
    for (const auto& e : list) {
      size_t cell = lg > 2 ? (size_t)((e.first * 0x9E3779B1u) >> (34 - lg)) : 0;
      unsigned dist = 1;
      for (;; cell = (cell + 1) & (cells - 1), dist++) {
        size_t at = off + 4 * cell, free_slot = 4;
        for (size_t m = 0; m < 4; m++)
          if (o.tkeys[at + m] == 0xFFFFFFFFu) {
            free_slot = m;
            break;
          }
        if (free_slot < 4) {
          o.tkeys[at + free_slot] = e.first;
          o.tslot[at + free_slot] = e.second;
          break;
        }
      }
      probes = std::max(probes, dist);
    }
    if (probes > 255) {   // (cannot happen below 100 % load; keeps the field in range)
      o.dir[2 * (size_t)key + 1] = SXMC_SPARSE_SLOW;
      continue;
    }
    lg |= (int)(probes << 8);
    o.dir[2 * (size_t)key] = (unsigned)off;
    o.dir[2 * (size_t)key + 1] = (unsigned)lg;
  }
}

// ---------------------------------------------------------------------------------------------- event classes
// Events with the same bin (or counter slot) in every member contribute the same term to the event sum
// (nll_kernels.cpp:101-112), so the sum runs over the K distinct tuples, each weighted by its multiplicity.
// arr[j]: member j's table, one entry per event (E entries each).  tables[j * K + k] = member j's entry of class k.
struct EventClasses {
  size_t K = 0;
  std::vector<unsigned> first, weight;   // per class: an event that belongs to it; how many do
  std::vector<int> tables;
};

inline void event_classes(const std::vector<const std::vector<int>*>& arr, size_t E, EventClasses& o) {
  const size_t S = arr.size();
  // members with identical tables (one binning, one data set: the usual case) count once in the key
  std::vector<int> distinct;
  for (size_t j = 0; j < S; j++) {
    bool seen = false;
    for (size_t q = 0; q < distinct.size() && !seen; q++) seen = *arr[(size_t)distinct[q]] == *arr[j];
    if (!seen) distinct.push_back((int)j);
  }
  std::vector<unsigned> order(E);
  for (size_t i = 0; i < E; i++) order[i] = (unsigned)i;
  auto less = [&](unsigned a, unsigned b) {
    for (int q : distinct) {
      const int x = (*arr[(size_t)q])[a], y = (*arr[(size_t)q])[b];
      if (x != y) return x < y;
    }
    return false;
  };
  auto same = [&](unsigned a, unsigned b) {
    for (int q : distinct)
      if ((*arr[(size_t)q])[a] != (*arr[(size_t)q])[b]) return false;
    return true;
  };
  std::sort(order.begin(), order.end(), less);
  o.first.clear();
  o.weight.clear();
  for (size_t i = 0; i < E; i++) {
    if (i > 0 && same(order[i - 1], order[i])) {
      o.weight.back()++;
    } else {
      o.first.push_back(order[i]);
      o.weight.push_back(1u);
    }
  }
  o.K = o.first.size();
  o.tables.assign(std::max<size_t>(S * o.K, 1), 0);
  for (size_t j = 0; j < S; j++)
    for (size_t k = 0; k < o.K; k++) o.tables[j * o.K + k] = (*arr[j])[o.first[k]];
}

// Real event weights over the classes above: W[k] = the sum of w[i] over the events i of class k, in ASCENDING EVENT
// INDEX, in double, added one by one from 0.0 -- the order is the law (tests/weighted_events_reference.py), not
// event_classes' sort, which is not stable.  All weights 1.0 give W[k] == (double)weight[k] exactly; integer weights give
// the multiplicities of the data set with event i repeated w[i] times.  `arr`, `E`: what `cls` was built from.
inline void class_weights(const std::vector<const std::vector<int>*>& arr, size_t E, const EventClasses& cls,
                          const double* w, std::vector<double>& W) {
  W.assign(cls.K, 0.0);
  // (the classes are in the sort's order of their keys: an event finds its own by bisection over their first events)
  auto less = [&](unsigned a, unsigned b) {
    for (const std::vector<int>* t : arr) {
      const int x = (*t)[a], y = (*t)[b];
      if (x != y) return x < y;
    }
    return false;
  };
  for (size_t i = 0; i < E; i++) {
    const size_t k = (size_t)(std::lower_bound(cls.first.begin(), cls.first.end(), (unsigned)i, less) - cls.first.begin());
    W[k] = W[k] + w[i];
  }
}

// The first event weight that is not a finite double >= 0, or -1: sxmc_group_set_event_weights refuses by this index.
inline long long first_bad_event_weight(const double* w, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (!(w[i] >= 0.0) || w[i] > 1.7976931348623157e308) return (long long)i;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------------- mixed columns
// sxmc_group_set_columns: the walk's columns in signal order, member_of_signal[j] >= 0 a member of the group, -1 a dense
// column somebody else writes.  Valid: nothing below -1 or beyond the last member, every member exactly once.  Returns
// null, or what is wrong.
inline const char* columns_error(int nmembers, int nsignals, const int* member_of_signal) {
  if (nmembers < 0 || nsignals < 1 || !member_of_signal) return "set_columns: no columns";
  std::vector<int> seen((size_t)nmembers, 0);
  for (int j = 0; j < nsignals; j++) {
    const int m = member_of_signal[j];
    if (m < -1 || m >= nmembers) return "set_columns: a column names no member of the group";
    if (m >= 0 && seen[(size_t)m]++) return "set_columns: a member appears in two columns";
  }
  for (int m = 0; m < nmembers; m++)
    if (!seen[(size_t)m]) return "set_columns: a member appears in no column";
  return nullptr;
}

// CODES (fill_ordered_body): the window [base, base + 65532 step] of every streamed field of an ordered table, from the
// fields' finite ranges in the table (minmax[2m], minmax[2m + 1]; min > max: no finite value) and the domains of the
// observables among them (fields 0 .. nobs-1).  An observable's window is its finite range cut to its domain widened by
// its own width on either side -- a value further out needs a scale or shift of the order of the whole domain to come
// back in, and its row is marked "ask the exact columns" instead; a field that is only read gets its finite range, cut
// to three widths of the observables' windows around them when the two overlap at all.  step > 0 and finite, always.
struct CodeWindows {
  std::vector<double> base, step;
};
inline void code_windows(const float* minmax, int nfields, int nobs, const double* lower, const double* upper,
                         CodeWindows& o) {
  o.base.assign((size_t)nfields, 0.0);
  o.step.assign((size_t)nfields, 1.0);
  double ulo = 0, uhi = -1;   // union of the observables' windows
  for (int m = 0; m < nfields; m++) {
    double wlo = minmax[2 * m], whi = minmax[2 * m + 1];
    const bool none = !(wlo <= whi);
    if (m < nobs) {
      const double lo = lower[m], hi = upper[m], w = hi - lo;
      wlo = none ? lo - w : std::max(wlo, lo - w);
      whi = none ? hi + w : std::min(whi, hi + w);
      if (!(wlo < whi)) {   // (no finite value near the domain)
        wlo = lo - w;
        whi = hi + w;
      }
      if (uhi < ulo) {
        ulo = wlo;
        uhi = whi;
      } else {
        ulo = std::min(ulo, wlo);
        uhi = std::max(uhi, whi);
      }
    } else if (none) {
      wlo = 0;
      whi = 1;
    } else if (ulo <= uhi) {
      const double w = uhi - ulo, clo = std::max(wlo, ulo - 3 * w), chi = std::min(whi, uhi + 3 * w);
      if (clo < chi) {
        wlo = clo;
        whi = chi;
      }
    }
    double step = (whi - wlo) / 65532.0;   // (the largest value lands in code 65532 of 0 .. 65533)
    if (!(step > 0) || !std::isfinite(step)) step = std::max(std::fabs(wlo), 1.0) * 0x1p-20;
    o.base[(size_t)m] = wlo;
    o.step[(size_t)m] = step;
  }
}

// LDS of fill_ordered_body (histograms in LDS): 4 header words, per chain 2^rlog replicas `rstride` words apart, 64
// spare words, then the queues of the codes path: 4 words + 2 per entry, (1 << qlog) entries shared out over the waves.
inline unsigned ordered_rstride_plain(int max_bins) { return (((unsigned)max_bins + 63u) & ~63u) + 16u; }
// ... in the padded form the codes path uses when ONE observable is binned per sample and it is the histogram's
// outermost dimension: (nbins + 2) rows of S' words, S' = S | 1 (odd: lanes that differ in the index hit different
// banks), a guard row either side; + 16 mod 64 like the plain form (a bin's replicas in different banks)
inline unsigned ordered_rstride_padded(int total_bins, int outer_bins) {
  const unsigned S = (unsigned)(total_bins / outer_bins), Sp = S | 1u;
  const unsigned words = ((unsigned)outer_bins + 2u) * Sp;
  return ((words + 63u) & ~63u) + 16u;
}
inline size_t ordered_queue_bytes(unsigned qlog) { return qlog ? (4 + ((size_t)2 << qlog)) * 4 : 0; }
inline size_t ordered_lds_bytes(unsigned rstride, int nchain, unsigned rlog) {
  return (4 + ((size_t)nchain * rstride << rlog) + 64) * 4;
}
constexpr unsigned kMinQueueLog = 9;     // the smallest queues of ambiguous rows a fill over codes works with: 2^9 entries
// the largest set of queues (512 .. 2048 entries: every wave of the workgroup owns an equal slice) that fits `room`
// bytes, as log2(entries); 0: none, the launch then streams the float columns
inline unsigned ordered_queue_log(size_t room, int cap = 0) {
  unsigned qlog = 11;
  // (sxmc_group_set_codes_queue_log caps the queues at 2^9 .. 2^11 entries -- smaller queues fill up and are emptied in
  // the middle of the stream, and whole granules are handed to the float columns; the results do not depend on it)
  if (cap > 0) qlog = (unsigned)std::min(std::max(cap, (int)kMinQueueLog), 11);
  while (qlog >= kMinQueueLog && ordered_queue_bytes(qlog) > room) qlog--;
  return qlog >= kMinQueueLog ? qlog : 0;
}

// The padded form's stride where every member of a launch qualifies (`descs`: the members as their fill sees them, one
// observable binned per sample in slot 0), else 0.  Ordered form: that observable must be the histogram's outermost
// dimension; the boxed form makes it the outermost dimension of the LDS copy wherever it sits.
inline unsigned padded_rstride_of(const std::vector<SxSignalDesc>& descs, bool boxed) {
  unsigned rs = 0;
  for (const SxSignalDesc& d : descs) {
    const long long nb = d.nbins[0], total = d.total_nbins;
    const long long S = boxed ? (nb >= 1 ? total / nb : 0) : d.bin_stride[0];
    bool ok = S >= 1 && nb >= 1 && S * nb == total && S * (nb + 2) < (1ll << 22);
    if (boxed) ok = ok && d.bin_stride[0] >= 1 && total % ((long long)d.bin_stride[0] * nb) == 0;
    if (!ok) return 0;
    rs = std::max(rs, ordered_rstride_padded((int)total, (int)nb));
  }
  return rs;
}

// The LDS of one workgroup of fill_ordered_body / fill_boxed_body, which decode `word` blindly: rstride | rlog << 24 |
// padded << 27 | qlog << 28.  As many replicas (up to 2^rlog_max) of the chains' histograms as `share` bytes hold; over
// codes the padded form where one was offered and fits with the smallest queues, then the queues of ambiguous rows in
// what the replicas leave (`queue_cap`: sxmc_group_set_codes_queue_log).  fits == false: not even one replica does.
struct OrderedLdsIn {
  int max_bins = 0, nchain = 1;  // the largest histogram of the launch; chains per pass (1 .. 4)
  unsigned padded_rstride = 0;   // padded_rstride_of(...); 0: not eligible
  bool codes = false;
  size_t share = 0;              // the workgroup's share of the CU's LDS, bytes
  unsigned rlog_max = 2;
  int queue_cap = 0;
};
struct OrderedLds {
  unsigned word = 0, rlog = 0, qlog = 0;
  bool padded = false, fits = false;
  size_t bytes = 0;
};
inline OrderedLds ordered_lds_layout(const OrderedLdsIn& in) {
  OrderedLds o;
  const size_t qreserve = in.codes ? ordered_queue_bytes(kMinQueueLog) : 0;   // (room for the smallest queues)
  unsigned rstride = ordered_rstride_plain(in.max_bins);
  if (in.codes && in.padded_rstride && ordered_lds_bytes(in.padded_rstride, in.nchain, 0) + qreserve <= in.share) {
    rstride = in.padded_rstride;
    o.padded = true;
  }
  while (o.rlog < in.rlog_max && ordered_lds_bytes(rstride, in.nchain, o.rlog + 1) + qreserve <= in.share) o.rlog++;
  o.bytes = ordered_lds_bytes(rstride, in.nchain, o.rlog);
  if (in.codes) {
    o.qlog = in.share > o.bytes ? ordered_queue_log(in.share - o.bytes, in.queue_cap) : 0;
    o.bytes += ordered_queue_bytes(o.qlog);
  }
  o.word = rstride | (o.rlog << 24) | (o.padded ? 1u << 27 : 0u) | (o.qlog << 28);
  o.fits = o.bytes <= in.share;
  return o;
}

// ------------------------------------------------------------------------------------- which form a table takes
// What the systematics of a member do to its slots (`d` as fill_desc fills it: slot k is observable k, the extra
// fields after them).  Worked out once; every choice below reads it.
struct SystUse {
  unsigned written = 0;   // slots some systematic writes
  unsigned truth = 0;     // slots read as a resolution scale's truth field
  // per observable: some systematic on it has more than one coefficient; ... or is not a shift, scale or cos-theta
  // scale; some resolution scale writes it; against which slot (-1: none, -2: more than one)
  bool many_coef[SXMC_MAX_NFIELDS] = {}, not_affine[SXMC_MAX_NFIELDS] = {}, has_res[SXMC_MAX_NFIELDS] = {};
  int truth_slot[SXMC_MAX_NFIELDS];
  // A program every systematic of which is a short polynomial can run as straight-line code: from the table of
  // kernels built into the library, or specialised at run time (sxmc_rtc.cpp).
  bool specialisable = false;
  bool is_written(int k) const { return (written >> k) & 1u; }
  bool is_truth(int k) const { return (truth >> k) & 1u; }
  // written by one-coefficient shift / scale / cos-theta scale only
  bool affine_only(int k) const { return is_written(k) && !many_coef[k] && !not_affine[k]; }
};
inline SystUse syst_use(const SxSignalDesc& d) {
  SystUse u;
  std::fill(u.truth_slot, u.truth_slot + SXMC_MAX_NFIELDS, -1);
  int ncoef = 0;
  u.specialisable = d.nsyst <= 8;
  for (int q = 0; q < d.nsyst; q++) {
    const SxSystOp& op = d.syst[q];
    const int k = op.obs_slot;
    ncoef += op.npars;
    u.specialisable = u.specialisable && op.npars >= 1 && op.npars <= SXMC_MAX_SYST_PARS;
    u.written |= 1u << k;
    u.many_coef[k] = u.many_coef[k] || op.npars != 1;
    u.not_affine[k] = u.not_affine[k] || !(op.type == SXMC_SYST_SHIFT || op.type == SXMC_SYST_SCALE || op.type == SXMC_SYST_CTSCALE);
    if (op.type == SXMC_SYST_RESOLUTION_SCALE) {
      u.truth |= 1u << op.extra_slot;
      u.truth_slot[k] = (!u.has_res[k] || u.truth_slot[k] == op.extra_slot) ? op.extra_slot : -2;
      u.has_res[k] = true;
    }
  }
  u.specialisable = u.specialisable && ncoef <= 16;
  return u;
}

// the program as words, one per systematic (the key of a launch class and of the kernel tables)
inline std::vector<unsigned> prog_words(const SxSignalDesc& x) {
  std::vector<unsigned> w;
  for (int q = 0; q < x.nsyst; q++) {
    w.push_back((unsigned)x.syst[q].type | ((unsigned)x.syst[q].obs_slot << 4) |
                ((unsigned)x.syst[q].extra_slot << 8) | (x.syst[q].npars > 1 ? (unsigned)x.syst[q].npars << 12 : 0u));
  }
  return w;
}

// buckets of a bucketed table: the bins of the observables no systematic writes
inline double unwritten_buckets(const SxSignalDesc& d, const SystUse& u) {
  double buckets = 1.0;
  for (int k = 0; k < d.nobs; k++) {
    if (!u.is_written(k)) buckets *= (double)d.nbins[k];
  }
  return buckets;
}

// (the runs kernel forms idx * stride + bin with ONE signed 24-bit multiply-add)
inline bool narrow_for_runs(const SxSignalDesc& d) {
  bool narrow = true;
  for (int k = 0; k < d.nobs; k++) narrow = narrow && d.nbins[k] < (1 << 23) && d.bin_stride[k] < (1 << 23);
  return narrow;
}

// The ORDERED observable: written by one-coefficient shift / scale / cos-theta scale only and read by nothing; of
// several, the one with the fewest bins (fewest granules that straddle an edge).  -1: none.  mode: 0 off, 1 where it
// pays, 2 wherever it applies.  A histogram beyond LDS (lds_hist false): only with the event-bin counters over runs
// (`runs_possible`: the caller's side of that -- evaluation points, room for the members' workgroups); the round-1
// filter path of a table left in sorted order has no ordered form.
inline int choose_ordered(const SxSignalDesc& d, const SystUse& u, int mode, bool lds_hist, bool runs_possible) {
  if (!mode || !(lds_hist ? d.total_nbins < (1 << 24) : (runs_possible && narrow_for_runs(d)))) return -1;
  int ordered = -1;
  for (int k = 0; k < d.nobs; k++) {
    if (u.affine_only(k) && !u.is_truth(k) && (ordered < 0 || d.nbins[k] < d.nbins[ordered])) ordered = k;
  }
  // Does it pay?  Up to nbins + 1 granules per bucket straddle an edge and stream everything; with fewer
  // than twice that many granules in all, most do (BASELINE config 5: 61 granules per bucket against 200
  // bins of r) and the ordered form only adds work.  mode == 2 (tests): wherever it applies.
  if (ordered >= 0 && mode == 1) {
    const double straddling = unwritten_buckets(d, u) * ((double)d.nbins[ordered] + 1.0);
    if ((double)d.nsamples / 256.0 < 2.0 * straddling) ordered = -1;
  }
  return ordered;
}

// The BOXED observable (fill_boxed_kernel): written by one-coefficient shift / scale / cos-theta scale and at least
// one resolution scale, all of those against ONE field that nothing writes, and read by nothing; beside it exactly one
// other written observable, with one-coefficient shift / scale / cos-theta scale only (one streamed field, as 16-bit
// codes).  Histogram in LDS.  Where the ordered form also applies this one streams half the bytes.  mode: 0 off, < 0
// where it pays, 1 wherever it applies; `strata`: strata of x - t inside a bucket.
struct BoxChoice {
  int obs = -1, truth = -1;   // the observable and the slot of its truth field; obs < 0: none
};
inline BoxChoice choose_boxed(const SxSignalDesc& d, const SystUse& u, int mode, int strata, bool lds_hist) {
  BoxChoice b;
  if (!mode || !lds_hist || d.total_nbins >= (1 << 22)) return b;
  int nwritten = 0;
  bool others_ok = true;
  for (int k = 0; k < d.nobs; k++) {
    if (!u.is_written(k)) continue;
    const bool ok = !u.many_coef[k] && u.truth_slot[k] != -2 && !u.is_truth(k);   // (is_truth: read by a systematic, itself included)
    nwritten++;
    if (u.has_res[k] && ok && b.obs < 0) {
      b.obs = k;
      b.truth = u.truth_slot[k];
    } else {
      others_ok = others_ok && ok && !u.has_res[k];
    }
  }
  const bool truth_written = b.truth >= 0 && u.is_written(b.truth);
  if (b.obs < 0 || nwritten != 2 || !others_ok || truth_written || d.nsyst > 8) return BoxChoice{};
  // Does it pay?  A box straddles an edge of the observable when it is not small against a bin: with fewer than a
  // few granules per bin, stratum and bucket most do.  mode == 1 (tests): wherever it applies.
  if (mode < 0) {
    const double per = (double)d.nsamples / 256.0 / (unwritten_buckets(d, u) * strata);
    if (per < 4.0 * ((double)d.nbins[b.obs] + 1.0)) return BoxChoice{};
  }
  return b;
}

// The member's problem as the fill sees it once its table is bucketed: only the observables some systematic
// writes (+ the extra fields), slots renumbered, columns = the bucketed copy.  `keep`: full slot -> new slot or -1.
// `ordered` >= 0: that observable rides in the last slot and its geometry at index nobs2 (fill_ordered_kernel).
inline void compact_desc(const SxSignalDesc& full, const std::vector<int>& keep, int nobs2, SxSignalDesc& cd, int ordered = -1) {
  cd = full;
  if (ordered >= 0) {
    cd.bin_stride[nobs2] = full.bin_stride[ordered];
    cd.nbins[nobs2] = full.nbins[ordered];
    cd.lower[nobs2] = full.lower[ordered];
    cd.upper[nobs2] = full.upper[ordered];
    cd.scale[nobs2] = full.scale[ordered];
  }
  int nslot = 0;
  for (int k = 0; k < full.nslot; k++) {
    if (keep[(size_t)k] < 0) continue;
    const int q = keep[(size_t)k];
    cd.slot_col[q] = q;  // the copy holds exactly the streamed fields, in slot order
    if (q < nobs2) {     // an observable the fill still bins (the others it keeps are read-only inputs)
      cd.bin_stride[q] = full.bin_stride[k];
      cd.nbins[q] = full.nbins[k];
      cd.lower[q] = full.lower[k];
      cd.upper[q] = full.upper[k];
      cd.scale[q] = full.scale[k];
    }
    nslot++;
  }
  cd.nobs = nobs2;
  cd.nslot = nslot;
  for (int q = 0; q < full.nsyst; q++) {
    cd.syst[q].obs_slot = (short)keep[(size_t)full.syst[q].obs_slot];
    cd.syst[q].extra_slot =
        (short)(full.syst[q].type == SXMC_SYST_RESOLUTION_SCALE ? keep[(size_t)full.syst[q].extra_slot] : 0);
  }
}

// Compacted slots of a bucketed table: the observables that are written (still binned by the fill), then everything
// that is only read -- the extra fields, and an untouched observable that serves as some systematic's truth field (its
// own bin index is the bucket's; its VALUE is still an input) --, then the ordered observable.  box_truth >= 0:
// `ordered` is a BOXED observable and box_truth the slot of its truth field.
struct CompactSlots {
  unsigned mask = 0;         // the observables the buckets are made of (those no systematic writes)
  unsigned pre_mask = 0;     // ... | 1 << (16 + ordered): the launch class's key
  std::vector<int> keep;     // full slot -> compacted slot or -1
  std::vector<int> fields;   // the table columns the copy streams, in compacted slot order
  int nobs2 = 0;             // observables the fill still bins per sample
  // a shape the ordered / boxed form takes.  The plain bucketed form (ordered < 0): one that has buckets and something
  // to bin; whether a kernel is specialised for (nobs2, fields.size()) is the caller's to ask.
  bool shape_ok = false;
};
inline CompactSlots compact_slots(const SxSignalDesc& d, const SystUse& u, int ordered, int box_truth, bool lds_hist) {
  CompactSlots c;
  c.keep.assign((size_t)d.nslot, -1);
  for (int k = 0; k < d.nobs; k++) {
    if (k == ordered) continue;
    if (u.is_written(k)) {
      c.keep[(size_t)k] = (int)c.fields.size();
      c.fields.push_back(d.slot_col[k]);
      c.nobs2++;
    } else {
      c.mask |= 1u << k;
    }
  }
  for (int k = 0; k < d.nslot; k++) {
    if (c.keep[(size_t)k] >= 0 || k == ordered) continue;
    if (k >= d.nobs || u.is_truth(k)) {
      c.keep[(size_t)k] = (int)c.fields.size();
      c.fields.push_back(d.slot_col[k]);
    }
  }
  if (ordered >= 0) {
    c.keep[(size_t)ordered] = (int)c.fields.size();
    c.fields.push_back(d.slot_col[ordered]);
  }
  c.pre_mask = c.mask | (ordered >= 0 ? 1u << (16 + ordered) : 0u);
  // (beyond LDS the granule word has no room for the row count: something must be binned per sample)
  c.shape_ok = box_truth >= 0 ? (c.nobs2 == 1 && c.fields.size() == 3 && lds_hist && c.fields[1] == d.slot_col[box_truth])
               : ordered >= 0 ? (c.nobs2 <= 5 && c.fields.size() <= 7 && (lds_hist || c.nobs2 >= 1))
                              : (c.mask && c.nobs2 >= 1);
  return c;
}

// pre-binning: the observables that no systematic writes as ONE narrow column of partial bin indices (1 or 2 bytes wide;
// width 0: none to pre-bin, or the index does not fit 16 bits)
struct PrebinColumns {
  unsigned mask = 0;
  int width = 0;
};
inline PrebinColumns prebin_columns(const SxSignalDesc& d, const SystUse& u) {
  PrebinColumns p;
  long long bound = 0;  // largest value the partial index can take (index == nbins included)
  for (int k = 0; k < d.nobs; k++) {
    if (!u.is_written(k)) {
      p.mask |= 1u << k;
      bound += (long long)d.nbins[k] * d.bin_stride[k];
    }
  }
  p.width = bound < 0xFF ? 1 : 2;
  if (!p.mask || bound >= 0xFFFF) return PrebinColumns{};
  return p;
}

}  // namespace sxplan
