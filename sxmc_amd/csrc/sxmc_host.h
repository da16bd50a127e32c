// sxmc_host.h -- what the translation units of libsxmc_hip.so's host side share: the handle structures behind the C ABI
// (include/sxmc_hip.h), the error and ordering macros every entry point starts with, and the functions one unit offers
// the others.  Internal.  The units, by concern:
//   sxmc_runtime.cpp      errors, tracing, device / memory / stream / graph / event entry points, the lazy EvalFinished's
//                         bookkeeping (settle), the capture gate
//   sxmc_launch_plan.cpp  a group's launch plans (LaunchPlan, one per form of the tables; the planner's steps take the group,
//                         a PlanConfig and the plan they fill): tables (bucketed copies, codes, sparse structures), launch
//                         classes, partitions, refresh; event classes; the fill launches (group_fill, over active_plan)
//   sxmc_evaluator.cpp    the evaluator (sxmc_hist_*) and the deferred batches behind its EvalAsync / EvalFinished
//   sxmc_group.cpp        the group entry points: configuration, autotune, evaluation, the step and its step-end forms
//   sxmc_multigroup.cpp   lockstep chains and the look-ahead pass
//   sxmc_nll_api.cpp      the NLL launch points with the reference's argument lists; the measurement build's test hooks
//   sxmc_kde.cpp          the kernel-density evaluator (sxmc_kde_*) behind pdfz::EvalKernel: creation, points, bindings,
//                         launch, streams, accessors (its state, shared with the next two: sxmc_kde_state.h)
//   sxmc_kde_cv.cpp       ... its bandwidth cross-validation
//   sxmc_kde_draw.cpp     ... what reads the last evaluation's rows: sampling and the projection
// The kernels, each file with its launchers:
//   pdfz_kernels.hip      zero, the fills (bodies: fill_kernels.inc.h) and their registry, PDF lookup, pre-binning, transposes
//     step_end_kernels.inc.h   ... and, in the same translation unit, the end of a step in all its forms
//                              (its grids, LDS size and ticket words: step_end_plan.h, pure)
//   nll_kernels.hip       the reference's separate NLL entry points (device parts: nll_device.h)
//   kde_kernels.hip, columns_kernels.hip, layout_kernels.hip, project_kernels.hip
// Every allocation these hold is owned by a buffer (device_buffer.h over the policies below); layout_kernels.hip's host
// helpers take their temporaries from the same type.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "device_buffer.h"
#include "sxmc_device.h"
#include "sxmc_plan.h"

extern "C" {
hipError_t sx_nll_init_rngs(int, int, hipStream_t, int, unsigned long long, sxmc_rng_state*);
hipError_t sx_nll_philox_dump(hipStream_t, sxmc_rng_state*, unsigned*, int);
hipError_t sx_nll_pick_new_vector(int, int, hipStream_t, int, sxmc_rng_state*, const float*, const double*,
                                  double*);
hipError_t sx_nll_jump_decider(int, int, hipStream_t, sxmc_rng_state*, double*, const double*, double*,
                               const double*, unsigned, int*, int*, float*);
hipError_t sx_nll_event_chunks(int, int, hipStream_t, const float*, const double*, size_t, size_t,
                               const double*, const unsigned*, const short*, const unsigned*, double*);
hipError_t sx_nll_event_chunks_weighted(int, int, hipStream_t, const float*, const double*, size_t, size_t,
                                        const double*, const unsigned*, const short*, const unsigned*, double*,
                                        const double*);
hipError_t sx_nll_event_reduce(int, hipStream_t, size_t, const double*, double*);
hipError_t sx_nll_total(hipStream_t, size_t, const double*, size_t, size_t, const double*, const double*,
                        const double*, const double*, const unsigned*, const short*, const unsigned*, double*,
                        const double*);
hipError_t sx_nll_finish_combo(int, hipStream_t, size_t, const double*, size_t, size_t, const double*,
                               const double*, sxmc_rng_state*, double*, double*, double*, double*, int*, int*,
                               float*, int, const float*, const double*, const unsigned*, const short*,
                               const unsigned*, const double*, const double*, bool);
}


// MEASUREMENT BUILD (make VARIANT=_measure EXTRA=-DSXMC_MEASURE=1): the kernels' `dbg` hooks, the entry points that set
// them and the environment switches that exist for A/B runs only.  The product library has none of them: measure_env()
// is the constant nullptr there, and what remains readable from the environment are documented defaults that the ABI
// can set too (SXMC_ROCTX, SXMC_CODES, SXMC_DEFER_EVAL, SXMC_LAZY_FINISH, SXMC_COOP_STEP_END, SXMC_FUSED_STEP).
#ifndef SXMC_MEASURE
#define SXMC_MEASURE 0
#endif

struct sxmc_group;
struct sxmc_hist;

namespace sxhost {

// ---- errors, tracing (sxmc_runtime.cpp)
extern thread_local std::string g_last_error;
extern thread_local bool t_capturing;                       // this thread is recording a HIP graph (sxmc_graph_begin_capture)
extern thread_local unsigned long long t_capture_epoch;     // one per recording
extern thread_local std::vector<sxmc_group*> t_capture_groups;   // groups launched in the current recording
int fail(int code, const std::string& msg);
inline const char* measure_env(const char* name) {
#if SXMC_MEASURE
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
bool tracing();
struct TraceRange {
  bool on;
  explicit TraceRange(const char* name) : on(tracing()) {
    if (on) roctxRangePushA(name);
  }
  ~TraceRange() {
    if (on) roctxRangePop();
  }
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;
};


}  // namespace sxhost

#define SX_HIP_STATUS_(e, text)                                                                                     \
  do {                                                                                                              \
    hipError_t _e = (e);                                                                                            \
    if (_e != hipSuccess) {                                                                                         \
      return ::sxhost::fail(SXMC_ERR_HIP, std::string(text) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +     \
                                              std::to_string(__LINE__) + ")");                                       \
    }                                                                                                               \
  } while (0)
// a call of the runtime: anything but a hipError_t does not compile
#define SX_HIP(expr) SX_HIP_STATUS_(expr, #expr)
// a buffer's alloc / grow / reset, which hands the runtime's status on as the int of device_buffer.h's policies
#define SX_BUF(expr) SX_HIP_STATUS_(::sxhost::buffer_status(expr), #expr)

#define SX_REQUIRE(cond, msg)                                  \
  do {                                                         \
    if (!(cond)) return ::sxhost::fail(SXMC_ERR_INVALID, msg); \
  } while (0)

namespace sxhost {
// Who owns device memory: a buffer as a member of the handle that uses it, or as a local for a temporary.  Freed when
// the owner dies; a hipFree stalls every stream of the device, so the grow-only members are never shrunk.
struct DeviceMem {
  static int allocate(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static int free(void* p) { return (int)hipFree(p); }
};
struct PinnedMem {
  static int allocate(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static int free(void* p) { return (int)hipHostFree(p); }
};
template <typename T>
using DeviceBuffer = sxbuf::Buffer<T, DeviceMem>;
template <typename T>
using PinnedBuffer = sxbuf::Buffer<T, PinnedMem>;
inline hipError_t buffer_status(int status) { return static_cast<hipError_t>(status); }   // (SX_BUF)

constexpr int kLdsMaxBins = 40960 - 128;  // 160 KiB of LDS per workgroup minus header and trash words

struct HostSyst {
  int type, obs, extra_field;
  std::vector<short> pars;
};

struct DeviceProps {
  int cus = 0;
  int lds_per_cu = 0;
  bool valid = false;
};

int get_props(DeviceProps& p);
}  // namespace sxhost

// The immutable part of an evaluator: the column-major sample table and (built on demand) the
// pre-binned column.  Shared by evaluators created with sxmc_hist_create_shared, so that several
// chains / experiments on one GPU read ONE copy of the MC tables.
struct SampleStore {
  sxhost::DeviceBuffer<float> d_cols;
  // pre-binned columns built so far, one per (observable mask, width); kept until the table dies because
  // descriptors of other groups may point at them
  struct PreColumn {
    unsigned mask;
    int width;
    sxhost::DeviceBuffer<void> ptr;
  };
  std::vector<PreColumn> pre;
  std::mutex pre_mutex;  // evaluators sharing the table may be set up from different host threads
  void* find_pre(unsigned mask, int width) const {
    for (const PreColumn& p : pre)
      if (p.mask == mask && p.width == width) return p.ptr.get();
    return nullptr;
  }
  // Bucketing (layout_kernels.hip).  The SORT of the rows by the untouched observables' bin indices is done once
  // per set of untouched observables (`mask`) and kept; `rejected`: it was tried and the padding of the granules
  // would have outweighed the columns saved (tiny tables with many buckets).
  struct BucketSort {
    unsigned mask = 0;
    int ordered = -1;               // observable whose raw value orders the rows inside every bucket, or -1
    int box_truth = -1;             // >= 0: `ordered` is a BOXED observable (fill_boxed_kernel) and this the truth field
                                    // its resolution scale reads: rows of a bucket go by (stratum of x - t, x)
    bool rejected = true;
    sxhost::DeviceBuffer<unsigned> d_rows;   // [nsamples] row numbers in sorted order (rows outside the domain last)
    size_t nkept = 0;               // rows inside the domain of every untouched observable
    unsigned nkeys_total = 0;       // size of the key space (= the key of "outside")
    unsigned radix[SXMC_MAX_NFIELDS] = {0};
    std::vector<unsigned> keys;     // bucket keys present, ascending
    std::vector<unsigned> key_pre;  // bin offset of each of them
    std::vector<unsigned> lsrc, lvalid, lwhich;  // logical granules: first sorted position, rows, index into keys
  };
  // ... and the COPIES laid out from it, one per (mask, streamed fields, runs); kept until the table dies because
  // descriptors of other groups may point at them.
  struct Bucketed {
    unsigned mask = 0;
    std::vector<int> fields;        // streamed fields, in the order of the compacted slots
    int runs = 1;                   // granule order transposed for this many runs (1 = sorted order)
    bool complete = false;
    const BucketSort* sort = nullptr;
    sxhost::DeviceBuffer<float> d_cols;     // [fields.size()][pitch]
    size_t pitch = 0;
    sxhost::DeviceBuffer<unsigned> d_gpre;  // [ngranules] bin offset of the granule
    sxhost::DeviceBuffer<unsigned> d_gkp;   // [ngranules] pairs {bucket key, bin offset}
    sxhost::DeviceBuffer<float> d_gedge;    // [ngranules] pairs {first, last} value of the sort's ordered observable
    sxhost::DeviceBuffer<float> d_gbox;     // [ngranules] {xmin, xmax, tmin, tmax} of the sort's boxed observable and its truth field
    double box_dx = 0, box_dt = 0;  // ... their mean extents over the granules with finite boxes
    bool q16 = false;               // d_qcol holds ONE 16-bit code per row of field 0 (boxed tables)
    size_t ngranules = 0;           // physical granules (with the runs' padding)
    size_t nkept = 0;               // samples in the copy
    // CODES (fill_ordered_body): the streamed fields once more as 16-bit codes, two per word; built on demand
    sxhost::DeviceBuffer<unsigned> d_qcol;  // [(nq + 1) / 2][pitch]
    int nq = 0;                     // fields coded (the streamed ones: all but the ordered observable's)
    bool codes_tried = false;
    double qbase[SXMC_MAX_QSLOTS] = {0}, qstep[SXMC_MAX_QSLOTS] = {0};
    unsigned long long q_exact_rows = 0, q_never_rows = 0;   // rows marked "ask the exact columns" / "never counted"
  };
  std::vector<std::unique_ptr<BucketSort>> sorts;
  std::vector<std::unique_ptr<Bucketed>> bucketed;
  BucketSort* find_sort(unsigned mask, int ordered, int box_truth = -1) const {
    for (const auto& b : sorts)
      if (b->mask == mask && b->ordered == ordered && b->box_truth == box_truth) return b.get();
    return nullptr;
  }
  Bucketed* find_bucketed(const BucketSort* sort, const std::vector<int>& fields, int runs) const {
    for (const auto& b : bucketed)
      if (b->sort == sort && b->fields == fields && b->runs == runs) return b.get();
    return nullptr;
  }
};

struct sxmc_hist {
  std::shared_ptr<SampleStore> store;
  int nfields = 0, nobs = 0;
  size_t nsamples = 0, nvec = 0, pitch = 0;
  unsigned dataset = 0;
  std::vector<double> lower, upper, scale;
  std::vector<int> nbins, stride;
  int total_nbins = 0;
  double bin_volume = 0;
  sxhost::DeviceBuffer<unsigned> d_bins;
  sxhost::DeviceBuffer<int> d_read_bins;   // (grow-only: a new data set of about the same size re-uses the buffer)
  std::vector<sxhost::DeviceBuffer<int>> retired;   // outgrown d_read_bins: other groups' descriptors may still point at
                                                    // them, so they are freed with the evaluator
  sxhost::DeviceBuffer<unsigned> d_cdf;    // prefix sums of the histogram, for sxmc_hist_random_sample
  sxhost::DeviceBuffer<void> d_sample;     // ... and the events drawn, a kernel-density evaluator's too (sxhost::sample_buffer;
                                           // grow-only: a fake experiment per walk draws about as many), bytes
  sxhost::DeviceBuffer<unsigned long long> d_marginal;   // sxmc_hist_project's totals along one observable (grow-only)
  bool has_points = false;
  size_t npoints = 0;
  float* pdf = nullptr;
  int pdf_off = 0, pdf_stride = 1;
  unsigned* norm = nullptr;
  int norm_off = 0;
  const double* params = nullptr;
  int par_off = 0, par_stride = 1;
  std::vector<sxhost::HostSyst> systs;
  hipStream_t stream = nullptr;
  unsigned long long version = 1;
  sxmc_group* self = nullptr;
  int cfg_threads = 0, cfg_bpc = 0;
  bool outputs_host_visible = false;   // a bound output (norm, pdf values) lies in memory the host reads directly
  bool want_optimize = true;       // EvalHist's `optimize` (pdfz.cpp:188, 441-448): trial launches at the first evaluation
  // sparse counting (histogram too large for LDS): one counter per distinct event bin
  sxhost::DeviceBuffer<unsigned> d_cnt;    // [ntargets]
  sxhost::DeviceBuffer<int> d_read_slot;   // [npoints]: counter slot of each event, or -1 / -2
  sxhost::DeviceBuffer<unsigned> d_filter;
  sxhost::DeviceBuffer<unsigned> d_table;
  sxhost::DeviceBuffer<unsigned> d_coarse; // coarse filter staged in LDS by the fill kernel
  int ntargets = 0, filter_shift = 0, table_shift = 0, coarse_shift = 0;
  // the event bins grouped by bucket, for sparse counting over a bucketed table walked in runs (fill_sparse_kernel)
  sxhost::DeviceBuffer<unsigned> d_bdir;   // [nkeys + 1] pairs {first table entry, log2 size | flag}
  sxhost::DeviceBuffer<unsigned> d_btkeys;
  sxhost::DeviceBuffer<unsigned> d_btslot;
  unsigned btab_mask = 0;
  unsigned long long btab_points_version = 0;
  bool btab_valid = false;
  std::vector<unsigned> targets;   // sorted distinct event bins (host copy: members with equal sets share tables)
  std::vector<int> h_read_bins;    // host copies of d_read_bins / d_read_slot: the group forms event classes from them
  std::vector<int> h_read_slot;
  unsigned long long points_version = 0;
  bool bins_valid = true;          // false after a sparse evaluation: the dense histogram was not filled
  const sxmc_group* cleared_by = nullptr;  // the group whose finish_step cleared this histogram and nothing has
                                           // counted into it since (any group's fill resets it)
  // sxmc_hist_set_sample_multiplicities: one `unsigned` per table row, padded with 0 to `pitch` words (the weighted fill
  // reads whole 4-row units); shared with the evaluators made from this one (sxmc_hist_create_shared).  Null: every row
  // counts once.  Set before the evaluator joins a group (`joined`: any evaluation goes through one) and not afterwards.
  std::shared_ptr<sxhost::DeviceBuffer<unsigned>> mult;
  unsigned long long mult_total = 0;   // sum of the multiplicities (<= 2^32 - 1)
  bool joined = false;
  // sxmc_hist_eval_async defers (see "deferred evaluations" below)
  std::shared_ptr<struct DeferredBatch> deferred;  // the host thread's batch of evaluations not launched yet it sits in
  std::shared_ptr<struct BatchInFlight> inflight;  // the batched launch the last sxmc_hist_eval_async went into
  ~sxmc_hist() {   // (releases only: what must happen before them is sxmc_hist_destroy's)
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// A host thread's evaluations asked for and not launched yet (sxmc_hist_eval_async).  Filled and launched by its
// thread only; another thread may only take an evaluator OUT of it (sxmc_hist_destroy), under the mutex.
struct DeferredBatch {
  std::mutex m;
  std::vector<sxmc_hist*> members;
  std::atomic<size_t> n{0};                // members.size(), readable without the mutex
  int do_eval_pdf = 0;
  std::thread::id owner;
};

// One batched launch of deferred evaluations: the stream it went to, and whether some member's EvalFinished has
// already waited for it (the siblings' EvalFinished then return at once: S - 1 runtime calls saved per step).
struct BatchInFlight {
  hipStream_t stream = nullptr;
  std::atomic<bool> done{false};
  bool host_visible = false;   // some member writes its results where the host reads them directly: EvalFinished waits
};


namespace sxhost {
struct LaunchClass {
  SxLaunchShape shape;
  std::vector<unsigned> prog;  // one word per systematic when every one has a single coefficient
  bool prog_simple = false;
  unsigned pre_mask = 0;       // observables no systematic writes, streamed as one pre-binned column
  std::vector<int> member_idx;
  DeviceBuffer<SxSignalDesc> d_descs;
  DeviceBuffer<SxSignalDesc> d_descs_sparse;  // same members, sparse flavour (global-histogram classes)
  DeviceBuffer<SxSegment> d_segs;
  DeviceBuffer<unsigned> d_blk_off;
  unsigned long long total_vec = 0;
  int partition = 0;  // 1 sliced, 2 interleaved (what build_partition chose)
  bool light = false; // a pure stream: runs best with few waves per CU (see class_waves_per_cu)
  bool runs_mode = false;  // bucketed tables laid out in per-wave runs; the sparse flavour runs fill_sparse_kernel
  int teams = 1;           // teams of workgroups per member over a bucketed table (sxplan::interleaved_segments)
  bool codes = false;      // ordered tables: the streamed columns go as 16-bit codes (fill_ordered_body's CODES)
  bool dual = false;       // boxed tables with the ordered plan beside them (sxmc_group::ordered, sxmc_group_adapt_fill_form)
  float box_dx = 0, box_dt = 0;   // ... mean extents of the members' granule boxes, what the choice is made from
  int box_obs = -1, box_truth = -1;   // ... the boxed observable and its truth field, as slots of the members' full descriptors
  unsigned padded_rstride = 0;  // ... with the LDS histogram in the padded form: words between its replicas (0: not)
  int max_bins = 0;             // the largest histogram of the members
  // (shape.weighted: the members carry sample multiplicities -- part of the class's key, find_class)
};

// The settings a group's launch plan depends on: a plan built with other values than these is out of date (group_refresh).
struct PlanConfig {
  int threads = 0, bpc = 0;   // launch shape set by hand (0: the plan's own)
  int partition = 0;          // 0 auto, 1 sliced, 2 interleaved
  int teams = 0;              // teams per member over a bucketed table (0 = 1, the default)
  int prebin = 1;             // pre-bin the observables no systematic writes
  int bucket = 1;             // stream a bucketed copy of the table where that pays
  int order = 1;              // ... with the rows of a bucket ordered by a monotonically written observable
  int box = -1;               // ... or grouped into boxes of a two-field observable (-1: where it pays, 1: wherever it applies)
  int rtc = 1;                // specialise the fill kernel at run time for programs not built in
  int codes = -1;             // ordered tables streamed as 16-bit codes (-1: SXMC_CODES, default on)
  int queue_log = 0;          // ... cap on the queues of ambiguous rows, log2(entries) (0: what fits)
  int fused = -1;             // the whole step in ONE launch where the fill has that form (-1: SXMC_FUSED_STEP, default OFF: measured slower)
  bool operator==(const PlanConfig& o) const {
    return threads == o.threads && bpc == o.bpc && partition == o.partition && teams == o.teams && prebin == o.prebin &&
           bucket == o.bucket && order == o.order && box == o.box && rtc == o.rtc && codes == o.codes &&
           queue_log == o.queue_log && fused == o.fused;
  }
};

// What one pass of the planner produces for one form of the members' tables (sxmc_launch_plan.cpp).  What does not
// depend on the form -- the members, their descriptors in member order -- is the group's, once.
struct LaunchPlan {
  std::vector<LaunchClass> classes;
  std::vector<const SampleStore::Bucketed*> member_bucket;  // per member: the copy its fill streams, or null
  std::string note;              // why a launch of the plan took a slower general path (for launch_info)
  bool order_blocked = false;    // ordered tables beyond LDS could not be laid out in runs: planned without.  Never cleared.
  bool box_blocked = false;      // boxed tables found no room for their codes / LDS form, or no ordered plan beside them: ditto.  Cleared by sxmc_group_set_boxes only.
  void clear() { classes.clear(); member_bucket.clear(); note.clear(); }   // (the flags stay: they say what not to try again)
};
}  // namespace sxhost

struct sxmc_group {
  std::vector<sxmc_hist*> members;
  std::vector<unsigned long long> seen;
  std::vector<unsigned long long> seen_points;   // members' points_version at the last (re)plan
  std::vector<SxSignalDesc> h_descs;
  sxhost::DeviceBuffer<SxSignalDesc> d_descs;  // member order: zero / eval kernels
  sxhost::DeviceBuffer<SxSignalDesc> d_descs_sparse;  // member order, sparse flavour where a member supports it
  bool sparse_ready = false;        // some member has sparse structures and all of those have points
  int max_bins_sparse = 0;
  int cfg_sparse = 1;               // count only the event bins when evaluating for lookup
  sxhost::PlanConfig plan_cfg, plan_cfg_seen;      // the settings the plan depends on, and those the current plan was built with
  sxhost::LaunchPlan plan;                         // the plan of plan_cfg
  sxhost::LaunchPlan ordered;                      // ... and, where that one is boxed and plan_cfg.box < 0, the same members planned in
                                                   // the ORDERED form (plan_cfg with box = 0); empty whenever the plan has one form
  int fill_form = 2;                               // 1: the boxed plan's launches, 2: the ordered plan's (where there are two forms)
  sxhost::PinnedBuffer<double> h_pin;              // pinned host words sxmc_group_adapt_fill_form reads the parameters into
  unsigned adapt_tick = 0;                         // deferred batches launched for this group (every 256th asks for the form)
  float box_limit = 0.12f;                         // sxmc_group_adapt_fill_form: boxed while the image of a mean box is narrower (bins)
  std::string rtc_note;                            // why a run-time specialisation could not be had (last failure)
  int cfg_tail = 1;                                // sxmc_group_step_async: the one-workgroup step end where it fits
  bool tuned = false;                              // a deferred batch's group: the launch-shape trials have run
  int trial_launches = 0;                          // fills sxmc_group_optimize has launched for this group (all calls)
  int cfg_coop = -1;                               // ... and the cooperative one-launch step end (-1: SXMC_COOP_STEP_END, default on)
  int coop_fits = -1;                              // ... decided at the group's first step: do the step ends of all chains
                                                   //     stepping in this process fit the device many times over?
  int last_step_launches = 0;                      // kernels the last sxmc_group_step_async launched
  unsigned long long plan_generation = 0;          // counts launch plans built (a multigroup re-validates on change)
  int debug_mode = 0;
  const double* proposal_factor = nullptr;         // sxmc_group_set_proposal_factor: borrowed, P x P doubles, or null (diagonal)
  const double* constraint_whitening = nullptr;    // sxmc_group_set_constraint_whitening: borrowed, P x P doubles, or null (independent)
  // measurement build only (the gated step): the stream this group's NEXT step puts its fill on, beside the step end of
  // the step before (null: the step is launched on one stream, as always), and the step's index inside its recording
  hipStream_t split_fill_stream = nullptr;
  int split_node = 0;
  std::vector<hipEvent_t> split_events;
  int max_bins = 0;
  unsigned long long max_points = 0;
  bool same_points = false;
  hipStream_t last_stream = nullptr;
  bool built = false;
  // Events grouped by their tuple of bins over the members (used when the lookup table is not wanted,
  // cfg_lut == 0): one row per distinct tuple, weighted by how many events share it.  One set per descriptor
  // flavour (dense bins / sparse counter slots).
  struct EventClasses {
    sxhost::DeviceBuffer<int> d_rb;             // [nmembers][K] (grow-only, like d_weight)
    sxhost::DeviceBuffer<unsigned> d_weight;    // [K]
    sxhost::DeviceBuffer<double> d_real_weight; // [K] with event weights set: the classes' weight sums (sxplan::class_weights)
    sxhost::DeviceBuffer<SxSignalDesc> d_descs; // member descriptors reading the class tables, no lookup-table output
    SxStepEndTable table;                       // the same descriptors as the cooperative step end takes them by value,
    bool has_table = false;                     // ... built with every upload of d_descs (up to 16 members)
    size_t K = 0;
    bool tables_valid = false, descs_valid = false;
    std::vector<unsigned long long> seen_points;
  };
  EventClasses ec[2];               // [0] dense, [1] sparse flavour
  // sxmc_group_set_event_weights: one real weight per event (finite, >= 0), the host's copy and the device's; empty: every
  // event counts once.  Rows that are classes carry the classes' sums (ec[].d_real_weight), rows that are events these.
  std::vector<double> event_weights;
  sxhost::DeviceBuffer<double> d_event_weights;
  std::vector<SxSignalDesc> h_descs_sparse;
  int cfg_lut = 1;
  // sxmc_group_set_columns: the lookup table of a mixed fit in signal order, per column the member looked up in place or
  // -1 for a dense column somebody else writes; uploaded there, once (the step entries neither copy nor allocate)
  std::vector<int> col_member;
  sxhost::DeviceBuffer<int> d_col_member;
  // sxmc_group_finish_step_async zeroes histograms and normalisations for the next evaluation: that
  // evaluation then skips its zero kernel.  0 = nothing pre-zeroed, 1 = dense flavour, 2 = sparse flavour.
  int prezeroed = 0;
  bool last_sparse = false;
  unsigned long long capture_epoch = 0;  // last recording this group launched in
  sxhost::DeviceBuffer<unsigned> d_ticket;  // the step ends' sxstep::kTicketWords words (the ticket, zeroed by the zero kernel; timeouts; ...)
  sxhost::DeviceBuffer<double> d_step_sums; // 1024 partial sums of the fused step
  std::vector<char> h_tail;          // fused step (fill_step_kernel): the step end's arguments, passed to the kernel by value
  sxhost::DeviceBuffer<unsigned long long> d_coop_slots;  // cooperative step end: one hand-over slot per worker (step_end_kernel)
  sxhost::DeviceBuffer<double> d_coop_last;               // ... and the last partial of each that was not NaN
  // profiling of the fill kernel
  bool prof = false;
  std::vector<hipEvent_t> ev0, ev1;
  int prof_n = 0;
  ~sxmc_group() {   // (releases only: what must happen before them is sxmc_group_destroy's)
    for (hipEvent_t e : ev0) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev1) (void)hipEventDestroy(e);
    for (hipEvent_t e : split_events) (void)hipEventDestroy(e);
  }
};


struct sxmc_multigroup {
  std::vector<sxmc_group*> groups;
  std::vector<void*> fill_fn;        // per launch of the plan: the lockstep kernel (hipFunction_t)
  std::vector<size_t> lds_bytes;
  std::vector<unsigned> fill_w;          // the kernels' layout argument: words per histogram, or the ordered fill's replica layout
  std::vector<unsigned long long> seen;  // the groups' plan generations the kernels were chosen for
  std::string why_not;               // set when the chains cannot be stepped together
  bool joint_ends = true;            // the chains' step ends share two launches (sx_launch_chain_ends)
};


namespace sxhost {

// ---- the launch plan (sxmc_launch_plan.cpp)
using sxplan::kMinQueueLog;
using sxplan::ordered_queue_bytes;
void member_slots(const sxmc_hist* h, std::vector<int>& slot_col);
int fill_desc(const sxmc_hist* h, SxSignalDesc& d);   // a member's descriptor: table, slots, systematics, bindings
void free_sparse(sxmc_hist* h);
int build_sparse(sxmc_hist* h, const std::vector<int>& rb);
bool fused_step_requested(const PlanConfig& cfg);
int group_refresh(sxmc_group* g);
// Has the plan two forms, and which one do the fills launch now?  Read behind a group_refresh: the ordered plan is
// emptied by every rebuild that leaves one form, so no setting needs asking again here.
inline bool has_two_forms(const sxmc_group* g) { return !g->ordered.classes.empty(); }
template <class Group>   // (sxmc_group or const sxmc_group)
auto& active_plan(Group* g) { return has_two_forms(g) && g->fill_form == 2 ? g->ordered : g->plan; }
// sample multiplicities among the group's members: how many carry them (0: none; members.size(): all)
inline size_t weighted_members(const sxmc_group* g) {
  size_t n = 0;
  for (const sxmc_hist* h : g->members) n += h->mult ? 1 : 0;
  return n;
}
int group_check_bound(sxmc_group* g, bool need_pdf);
int ensure_event_classes(sxmc_group* g, bool sparse);
int group_prepare_fill(sxmc_group* g, hipStream_t s, bool sparse);
int group_fill(sxmc_group* g, hipStream_t s, bool sparse = false);

// ---- deferred evaluations and the lazy EvalFinished (sxmc_evaluator.cpp, sxmc_runtime.cpp)
struct AutoGroup {
  std::vector<sxmc_hist*> members;
  sxmc_group* g = nullptr;
};
extern std::mutex g_auto_mutex;
extern std::vector<AutoGroup> g_auto_groups;     // groups made for batches of two or more (a single evaluator has h->self)
extern thread_local std::shared_ptr<DeferredBatch> t_deferred;
extern std::shared_mutex g_capture_gate;         // shared: a recording in progress; exclusive: a batch on its way to the legacy stream
int flush_deferred();
// (the lazy EvalFinished, sxmc_runtime.cpp: a batch on the legacy stream whose EvalFinished did not wait, per device)
constexpr int kMaxDevices = 64;
extern std::atomic<int> g_lazy_finish;
extern std::atomic<bool> g_unsettled[kMaxDevices];
int current_device_slot();
bool lazy_finish_enabled();
bool host_can_read(const void* p);
int settle();
int settle_for(hipStream_t s);
// (the buffer sxmc_hist_random_sample and sxmc_kde_random_sample draw into, h->d_sample: `nobserved` rows of `row`
//  floats, then the count of events never accepted)
// room for a draw, the count cleared on h->stream:
int sample_buffer(sxmc_hist* h, size_t nobserved, size_t row, float*& d_events, unsigned*& d_exhausted);
// waits for the draw, then fails with "<count> of <nobserved> events could not be drawn ... each" + why, or copies out:
int sample_read_back(sxmc_hist* h, size_t nobserved, size_t row, const char* why, float* h_events);

// ---- the step and its end (sxmc_group.cpp)
extern std::atomic<int> g_stepping_groups;       // groups of this process that have stepped a chain (see note_stepping)
using sxstep::kCoopMaxWorkers;
using sxstep::step_sum_blocks;
// the kernels' argument pack from the public one; nsignals: the columns finish_nll_jump_pick_combo runs over
SxStepArgs sx_step_args(const sxmc_step_args& p, size_t nsignals, const double* factor = nullptr,
                        const double* whitening = nullptr);
// SXMC_ERR_SHAPE where a step end over these many parameters and signals cannot take the factor (its unstaged form)
int proposal_factor_check(const double* factor, int nparameters, size_t nsignals);
// the same for the correlated constraints' whitening matrix
int constraint_whitening_check(const double* whitening, int nparameters, size_t nsignals);
// The rows a step end walks: the event classes (their descriptors, events per class, K) or, with the lookup table
// wanted, the events themselves.  ensure_event_classes comes first, before anything is launched: the caller's.
struct StepRows {
  const SxSignalDesc* descs;
  const unsigned* weight;   // events per class, or null: rows are events
  unsigned long long ne;
  const double* real = nullptr;   // the group has event weights: one per row, in `weight`'s place
  // f(the rows' weights, in their type): the launchers of a row sum are templates over it
  template <typename F>
  auto with_weight(F&& f) const { return real ? f(real) : f(weight); }
};
StepRows step_rows(const sxmc_group* g, bool sparse);
// What an entry point does for its rows before anything is launched: the event weights' count against the members'
// points, and without the lookup table the event classes (ensure_event_classes).
int ensure_step_rows(sxmc_group* g, bool sparse);
void mark_cleared(sxmc_group* g, bool sparse);   // a step end has cleared this flavour's histograms and normalisations
bool step_end_takes_tail(const sxmc_group* g, bool sparse, unsigned long long ne);
void note_stepping(sxmc_group* g);
bool step_end_is_cooperative(const sxmc_group* g, unsigned long long ne);
int group_step_tail(sxmc_group* g, hipStream_t st, bool sparse, const StepRows& rows, const SxStepArgs& a);

}  // namespace sxhost

#define SX_ORDER(s)                                  \
  do {                                               \
    int _rc = ::sxhost::settle_for((hipStream_t)(s));          \
    if (_rc) return _rc;                             \
  } while (0)

#define SX_FLUSH()                                                          \
  do {                                                                      \
    if (::sxhost::t_deferred && ::sxhost::t_deferred->n.load(std::memory_order_relaxed) != 0) { \
      int _rc = ::sxhost::flush_deferred();                                           \
      if (_rc) return _rc;                                                  \
    }                                                                       \
  } while (0)


// For the library's other translation units that are not part of the host side proper (sxmc_comm.cpp)
int sx_flush_and_order(hipStream_t s);
