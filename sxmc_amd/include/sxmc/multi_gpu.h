// multi_gpu.h -- the ensemble of the reference (src/sxmc.cpp:44-145) over the GPUs of one node, driven from one
// process: a host thread per rank, experiment k on rank k mod G, ONE exchange of the intervals at the end.  How the
// experiments are shared out and the blocks of intervals are packed and put back in order is ensemble_plan.h (pure,
// tested without a device); how the rank threads meet before the collective is Rendezvous (lane_sync.h).
#pragma once

#include <atomic>
#include <chrono>
#include <exception>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "ensemble_plan.h"
#include "experiment.h"

namespace sxmc {

/** The runners' settings (experiment.h; `device` and `device_exclusive` are set per rank and ignored here) and what
 *  the ranks add. */
struct MultiGpuOptions : ExperimentOptions {
  unsigned nconcurrent = 4;       //!< experiments in flight per device when lockstep_chains < 2 (ensemble_concurrent)
  unsigned lockstep_chains = 4;   //!< >= 2: per device, lockstep sets of this many chains (ensemble_lockstep) ...
  unsigned lockstep_sets = 2;     //!< ... this many sets in flight
  /** How the per-device blocks of intervals meet.  RCCL: one ncclAllGather over xGMI -- the product path.
   *  HOST_STAGING: every device thread's block is copied into rank 0's buffer by the host.  It exists so that the
   *  G-thread logic (sharding, per-thread replicas, rendezvous, result order, medians, failure handling) can be
   *  rehearsed on a box with fewer cards than ranks -- RCCL refuses two ranks on one card -- and is never chosen by
   *  default. */
  enum Exchange { RCCL, HOST_STAGING } exchange = RCCL;
  double exchange_timeout_seconds = 120.0;   //!< a collective still pending after this long is aborted (fail fast)
  /** Which lock serialises set-up (allocation, uploads, launch plans, module loads), graph recording and tear-down of
   *  the device threads.
   *  PROCESS_WIDE (default): ONE lock for all cards -- a thread never allocates or synchronises a device while another
   *  thread records a graph or sets up, on whichever card.  No run on more than one card is on record yet, so the
   *  conservative lock is the default.
   *  PER_DEVICE: one lock per card for set-up and tear-down -- the cards' set-ups run side by side -- while GRAPH
   *  RECORDING stays exclusive for the whole process (RecordingGate: whoever records waits for every set-up section in
   *  the process to end, and new ones wait for the recording): only the paths that never record graphs are relaxed.
   *  With 16 experiments per card at 77 ms of set-up each, one lock for 8 cards serialises ~10 s of set-up against
   *  ~3.5 s of walking per card; this mode is what a real node is measured with (bench_cpp --per-device-locks, which
   *  bench.py's multi-GPU leg tries first).
   *  PER_RANK (tests): a lock per rank even when ranks share a card -- set-up on one host thread beside stepping and
   *  set-up of another on the SAME device, recording still exclusive: the concurrency PER_DEVICE allows between cards,
   *  exercised on a box with one. */
  enum Locking { PROCESS_WIDE, PER_DEVICE, PER_RANK } locking = PROCESS_WIDE;
  /** Called by every device thread (argument: its rank) when its experiments are done, before the rendezvous.
   *  May throw: the tests inject a failing rank with it. */
  std::function<void(size_t)> before_exchange;
};

struct MultiGpuEnsemble {
  std::vector<ExperimentResult> results;  //!< one per experiment, in experiment order (computed on its own GPU)
  std::vector<float> gathered;            //!< [nexperiments][nparameters][4] = point_estimate, lower, upper, coverage:
                                          //!< what rank 0 received through the RCCL all-gather, in experiment order
  std::vector<float> median_upper;        //!< per parameter: median over the experiments of the upper limit
  size_t nparameters = 0;
  int rccl_nranks = 0;                    //!< ncclCommCount of rank 0's communicator (0: host staging)
  std::vector<int> rccl_devices;          //!< ncclCommCuDevice of every rank's communicator
  std::vector<double> rank_seconds;       //!< per rank: replica set-up + its experiments, wall clock
  std::vector<double> rank_setup_seconds; //!< per rank: building its replica of the evaluators (upload + layout)
  /** per distinct device: the set-up lock of that card -- seconds its users waited for it (summed over the threads
   *  that asked), seconds it was held, acquisitions.  waited / (lanes x wall) is the serialised share of the run. */
  struct LockUse {
    int device;
    double waited_seconds, held_seconds;
    unsigned long long acquisitions;
  };
  std::vector<LockUse> setup_locks;
  /** how each device ran its experiments: "lockstep" (ensemble_lockstep) or "concurrent" (ensemble_concurrent) --
   *  also when lockstep was asked for and a kernel-density signal ruled it out (lockstep batches histogram fills; the
   *  lanes then walk the MIXED form, batched and recordable like a histogram fit's) */
  std::string device_mode;
};

namespace detail {

/** Device memory for floats, freed with its holder. */
class DeviceFloats {
 public:
  DeviceFloats() = default;
  ~DeviceFloats() { reset(); }
  DeviceFloats(const DeviceFloats&) = delete;
  DeviceFloats& operator=(const DeviceFloats&) = delete;
  void allocate(size_t n) {
    reset();
    check(sxmc_malloc((void**)&p, sizeof(float) * std::max<size_t>(n, 1)));
  }
  void reset() {
    if (p) sxmc_free(p);
    p = nullptr;
  }
  float* get() const { return p; }

 private:
  float* p = nullptr;
};

/** What a rank thread holds on its device: released under the rank's set-up lock, in this order, however the thread
 *  ends. */
struct RankResources {
  explicit RankResources(SetupLock& exclusive_) : exclusive(exclusive_) {}
  ~RankResources() {
    std::lock_guard<SetupLock> lock(exclusive);
    for (Signal& s : replica) delete s.histogram;
    send.reset();
    recv.reset();
    stream.reset();
  }
  SetupLock& exclusive;
  std::vector<Signal> replica;   //!< this rank's own evaluators, built from the host tables
  DeviceFloats send, recv;       //!< the all-gather's buffers (RCCL only)
  OwnedStream stream;            //!< ... and its stream
};

/** Throws `error` again as a pdfz::Error that says which rank it came from. */
[[noreturn]] inline void rethrow_for_rank(const std::exception_ptr& error, size_t r, int device) {
  const std::string who = "ensemble_multi_gpu: rank " + std::to_string(r) + " (device " + std::to_string(device) + "): ";
  try {
    std::rethrow_exception(error);
  } catch (const pdfz::Error& e) {
    throw pdfz::Error(who + e.msg);
  } catch (const std::exception& e) {
    throw pdfz::Error(who + e.what());
  } catch (...) {   // (a callback of the caller's may throw anything)
    throw pdfz::Error(who + "an exception that is neither a pdfz::Error nor a std::exception");
  }
}

/** One call of ensemble_multi_gpu: its arguments, and what its rank threads share. */
struct MultiGpuRun {
  typedef std::chrono::steady_clock Clock;
  const std::vector<int>& devices;
  unsigned long long base_seed;
  std::vector<Source>& sources;
  const std::vector<Signal>& signals;
  const std::vector<const std::vector<float>*>& tables;
  int nfields;
  std::vector<Systematic>& systematics;
  std::vector<Observable>& observables;
  unsigned nsteps;
  float burnin_fraction;
  const MultiGpuOptions& opt;
  ShardPlan plan;
  MultiGpuEnsemble& out;

  bool rccl = opt.exchange == MultiGpuOptions::RCCL, lockstep = false;
  std::vector<sxmc_comm_t> comms = std::vector<sxmc_comm_t>(plan.G, nullptr);
  std::vector<float> rank0 = plan.empty_blocks(plan.G);   //!< rank 0's copy of every rank's block
  std::vector<std::exception_ptr> errors = std::vector<std::exception_ptr>(plan.G);
  // one lock for the process, or one per card (ranks rehearsed on one card share theirs); key -1 = the process's
  std::map<int, SetupLock> locks{};
  RecordingGate gate{};   // recording anywhere excludes set-up everywhere (shared by the locks; see MultiGpuOptions)
  Rendezvous meet{plan.G};
  std::atomic<bool> give_up{false};   // a rank abandoned the exchange: the others stop waiting for it

  /** The RCCL communicators, and what they say about themselves. */
  void setup_comms() {
    if (!rccl) return;
    if (sxmc_comm_init_all(devices.data(), (int)plan.G, comms.data()) != SXMC_OK) {
      throw pdfz::Error(std::string("ensemble_multi_gpu: RCCL communicators: ") + sxmc_comm_last_error());
    }
    out.rccl_devices.assign(plan.G, -1);
    for (size_t r = 0; r < plan.G; r++) {
      int rk = -1, n = 0, dv = -1;
      if (sxmc_comm_query(comms[r], &rk, &n, &dv) == SXMC_OK) {
        out.rccl_devices[r] = dv;
        if (r == 0) out.rccl_nranks = n;
      }
    }
  }
  int lock_key(size_t r) const {
    return opt.locking == MultiGpuOptions::PER_DEVICE ? devices[r]
           : opt.locking == MultiGpuOptions::PER_RANK ? 1000 + (int)r : -1;
  }
  void pick_locks() {
    for (size_t r = 0; r < plan.G; r++) {
      locks.emplace(std::piecewise_construct, std::forward_as_tuple(lock_key(r)),
                    std::forward_as_tuple(opt.locking == MultiGpuOptions::PROCESS_WIDE ? nullptr : &gate));
    }
  }

  /** Rank r's share of the experiments on its replica: in flight either as lockstep sets (one pass over the tables per
   *  step and set) or each with its own evaluation (ensemble_concurrent, nconcurrent in flight). */
  std::vector<ExperimentResult> experiments_of_rank(size_t r, const std::vector<unsigned>& ks, std::vector<Source>& src,
                                                    std::vector<Signal>& replica, std::vector<Systematic>& sys,
                                                    std::vector<Observable>& obs, SetupLock& exclusive) const {
    ExperimentOptions mine = opt;
    mine.device = devices[r];
    mine.device_exclusive = &exclusive;
    if (!lockstep) {
      return ensemble_concurrent(ks, base_seed, src, replica, sys, obs, nsteps, burnin_fraction, opt.nconcurrent, mine);
    }
    if (!mine.graph_steps) mine.graph_steps = 10;
    return ensemble_lockstep(ks, base_seed, src, replica, sys, obs, nsteps, burnin_fraction, opt.lockstep_chains,
                             opt.lockstep_sets, mine);
  }

  /** Everything rank r does before the ranks meet: its replica, its experiments, its block of intervals (on the device
   *  too when RCCL carries it).  Throws what went wrong. */
  void compute_block(size_t r, RankResources& held, std::vector<float>& send) {
    const Clock::time_point t0 = Clock::now();
    check(sxmc_set_device(devices[r]));
    std::vector<Systematic> sys = systematics;
    std::vector<Observable> obs = observables;
    std::vector<Source> src = sources;
    {
      std::lock_guard<SetupLock> lock(held.exclusive);
      for (size_t j = 0; j < signals.size(); j++) {
        Signal s = signals[j];
        s.histogram = nullptr;
        s.par_arrays.clear();
        build_pdfz(s, *tables[j], nfields, obs, sys);
        held.replica.push_back(s);
      }
    }
    out.rank_setup_seconds[r] = std::chrono::duration<double>(Clock::now() - t0).count();
    const std::vector<unsigned> ks = plan.experiments_of(r);
    const std::vector<ExperimentResult> res = experiments_of_rank(r, ks, src, held.replica, sys, obs, held.exclusive);
    for (size_t i = 0; i < res.size(); i++) {
      out.results[ks[i]] = res[i];
      plan.pack(send, i, res[i].intervals);
    }
    out.rank_seconds[r] = std::chrono::duration<double>(Clock::now() - t0).count();
    if (rccl) {
      std::lock_guard<SetupLock> lock(held.exclusive);
      held.send.allocate(plan.block());
      held.recv.allocate(plan.G * plan.block());
      check(sxmc_stream_create_nonblocking(held.stream.put()));
      check(sxmc_memcpy_h2d(held.send.get(), send.data(), sizeof(float) * plan.block()));
    }
    if (opt.before_exchange) opt.before_exchange(r);
  }

  /** The one exchange of the multi-GPU path: rank r's block into rank 0's copy of all of them.  RCCL: the all-gather,
   *  then a wait WITHOUT blocking inside the runtime -- a peer that gave up, an asynchronous RCCL error or the time
   *  limit end it by throwing.  Host staging: the host copies (disjoint blocks). */
  void exchange(size_t r, RankResources& held, const std::vector<float>& send) {
    if (!rccl) {
      std::copy(send.begin(), send.end(), rank0.begin() + (std::ptrdiff_t)(r * plan.block()));
      return;
    }
    if (sxmc_comm_allgather_f32(comms[r], held.send.get(), held.recv.get(), plan.block(), held.stream.get()) != SXMC_OK) {
      throw pdfz::Error(std::string("all-gather of the intervals: ") + sxmc_comm_last_error());
    }
    const Clock::time_point w0 = Clock::now();
    for (;;) {
      int done = 0, failed = 0;
      check(sxmc_stream_query(held.stream.get(), &done));
      if (done) break;
      if (give_up.load()) throw pdfz::Error("all-gather of the intervals: abandoned, another rank failed in it");
      if (sxmc_comm_async_error(comms[r], &failed) == SXMC_OK && failed) {
        throw pdfz::Error(std::string("all-gather of the intervals: ") + sxmc_comm_last_error());
      }
      if (std::chrono::duration<double>(Clock::now() - w0).count() > opt.exchange_timeout_seconds) {
        throw pdfz::Error("all-gather of the intervals: not complete after " +
                          std::to_string(opt.exchange_timeout_seconds) + " s (rank " + std::to_string(r) + ")");
      }
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (r == 0) check(sxmc_memcpy_d2h(rank0.data(), held.recv.get(), sizeof(float) * plan.G * plan.block()));
  }

  /** Rank r's host thread.  Every rank arrives at the rendezvous, failed or not; the collective is entered by all
   *  ranks or by none. */
  void rank_thread(size_t r) {
    RankResources held(locks.find(lock_key(r))->second);   // (find does not modify the map)
    std::vector<float> send = plan.empty_blocks();
    bool ok = true;
    try {
      compute_block(r, held, send);
    } catch (...) {
      errors[r] = std::current_exception();
      ok = false;
    }
    if (!meet.arrive(ok)) return;
    try {
      exchange(r, held, send);
    } catch (...) {
      errors[r] = std::current_exception();
      give_up.store(true);
      // end the pending collective on this rank's device BEFORE its stream and buffers are released (releasing
      // them would wait for a kernel that waits for a peer)
      if (comms[r]) {
        sxmc_comm_abort(comms[r]);
        comms[r] = nullptr;   // (the destroy after the join skips it)
      }
    }
  }
};

}  // namespace detail

/** The ensemble of sxmc.cpp:44-145 over the GPUs of one node, driven from one process: a host thread per
 *  rank, rank r on devices[r]; every rank builds its own replica of the evaluators from the host tables
 *  (`tables[j]` = signal j's row-major samples, what build_pdfz takes); experiment k runs on rank k mod G, several in
 *  flight per device (lockstep sets or ensemble_concurrent); no data-path collective.  At the end each rank
 *  contributes its experiments' intervals to ONE RCCL all-gather (sxmc_comm_allgather_f32: interval.h:22-27 as
 *  4 floats per parameter, padded to equal blocks), and rank 0's copy gives the medians (sxmc.cpp:126-145,
 *  utils.h:76-90).  `signals`: name, dataset, source, nexpected of every signal (histogram ignored).
 *
 *  Failure: the ranks meet on the host before the collective (Rendezvous).  If any rank failed -- a bad table, an
 *  experiment that threw, an allocation -- NO rank enters the all-gather and the first error is rethrown.  A rank
 *  whose collective does not complete (a peer lost after the rendezvous, exchange_timeout_seconds, an asynchronous
 *  RCCL error) aborts its communicator (ncclCommAbort) instead of waiting: the call returns an error, never hangs.
 *  Locking: set-up, graph recording and tear-down are serialised by ONE lock for the process (MultiGpuOptions::locking;
 *  PER_DEVICE: the lock of their own card only). */
inline MultiGpuEnsemble ensemble_multi_gpu(const std::vector<int>& devices, unsigned nexperiments,
                                           unsigned long long base_seed, std::vector<Source>& sources,
                                           const std::vector<Signal>& signals,
                                           const std::vector<const std::vector<float>*>& tables, int nfields,
                                           std::vector<Systematic>& systematics, std::vector<Observable>& observables,
                                           unsigned nsteps, float burnin_fraction, const MultiGpuOptions& opt) {
  PoolScope pool;   // (see ensemble(): blocks are pooled per device)
  const size_t G = devices.size();
  if (G == 0 || tables.size() != signals.size()) throw pdfz::Error("ensemble_multi_gpu: bad arguments");
  if (opt.asimov) {
    throw pdfz::Error("ensemble_multi_gpu: the Asimov data set is ONE fit, and one fit needs one card: run it with ensemble");
  }
  size_t P = sources.size();
  for (const Systematic& s : systematics) P += s.npars;
  MultiGpuEnsemble out;
  detail::MultiGpuRun run{devices, base_seed, sources, signals, tables, nfields, systematics, observables, nsteps,
                          burnin_fraction, opt, ShardPlan{G, nexperiments, P}, out};
  run.setup_comms();
  out.nparameters = P;
  out.results.resize(nexperiments);
  out.rank_seconds.assign(G, 0.0);
  out.rank_setup_seconds.assign(G, 0.0);
  // lockstep sets batch the chains' histogram fills: a kernel-density signal runs its device's experiments as
  // ensemble_concurrent lanes instead.  Every such lane walks the MIXED form (mcmc.h): its histogram signals in their
  // group, its kernel-density signals on the lane's stream, no host wait between steps, recorded when graph_steps asks
  bool any_kernel = false;
  for (const Signal& s : signals) any_kernel = any_kernel || s.pdf == "kernel";
  run.lockstep = opt.lockstep_chains >= 2 && !any_kernel;
  out.device_mode = run.lockstep ? "lockstep" : "concurrent";
  run.pick_locks();
  std::vector<std::thread> threads;
  for (size_t r = 0; r < G; r++) threads.emplace_back([&run, r]() { run.rank_thread(r); });
  for (std::thread& th : threads) th.join();
  for (sxmc_comm_t c : run.comms)
    if (c) sxmc_comm_destroy(c);
  for (auto& kv : run.locks) {
    out.setup_locks.push_back({kv.first, kv.second.waited_seconds(), kv.second.held_seconds(), kv.second.count()});
  }
  for (size_t r = 0; r < G; r++)
    if (run.errors[r]) detail::rethrow_for_rank(run.errors[r], r, devices[r]);   // the first failing rank's error
  out.gathered = run.plan.unpack(run.rank0);
  out.median_upper = run.plan.median_upper(out.gathered, median<float>);
  return out;
}

/** The same with the options spelled out as arguments (round 2's signature). */
inline MultiGpuEnsemble ensemble_multi_gpu(const std::vector<int>& devices, unsigned nexperiments,
                                           unsigned long long base_seed, std::vector<Source>& sources,
                                           const std::vector<Signal>& signals,
                                           const std::vector<const std::vector<float>*>& tables, int nfields,
                                           std::vector<Systematic>& systematics, std::vector<Observable>& observables,
                                           unsigned nsteps, float burnin_fraction, unsigned nconcurrent,
                                           float cl = 0.9f, unsigned sync_interval = 10000, unsigned graph_steps = 0,
                                           unsigned lockstep_chains = 4, unsigned lockstep_sets = 2) {
  MultiGpuOptions opt;
  opt.cl = cl;
  opt.sync_interval = sync_interval;
  opt.graph_steps = graph_steps;
  opt.nconcurrent = nconcurrent;
  opt.lockstep_chains = lockstep_chains;
  opt.lockstep_sets = lockstep_sets;
  return ensemble_multi_gpu(devices, nexperiments, base_seed, sources, signals, tables, nfields, systematics,
                            observables, nsteps, burnin_fraction, opt);
}

}  // namespace sxmc
