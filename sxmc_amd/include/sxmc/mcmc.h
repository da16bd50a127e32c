// mcmc.h -- ROOT-free MCMC driver in the shape of the reference's MCMC class (src/mcmc.{h,cpp}): the
// caller of the hot path.  Same constructor arguments and call operator; the chain comes back as a
// plain table (sxmc::Chain) instead of a TNtuple wrapped in a LikelihoodSpace.
//
// What it does per step (mcmc.cpp:261-348): re-evaluate every signal's PDF at the proposed vector
// (when systematics float), event log-sum, then the fused reduce + nll_total + Metropolis + next
// proposal.  Here the S evaluators are stepped as ONE batched launch sequence through
// sxmc_group_eval_nll_async (zero; fill of all signals in one kernel; lookup fused with the event sum)
// followed by the fused step end -- 4 launches per step instead of the reference's 3*S + 2.  `reference_form = true` issues the
// reference's own sequence of entry points instead (per-evaluator EvalAsync/EvalFinished,
// nll_event_chunks, finish_nll_jump_pick_combo); both forms give the same numbers up to the
// summation order of the event partial sums.
//
// A fit with kernel-density signals (pdfz::EvalKernel) among its histograms walks the MIXED form: the kernel members
// that read a floating parameter are evaluated on the walk's own stream, the histogram members form the group, the event
// sum runs over both kinds of column, and the step end clears the group only (Walk::mixed_step) -- no host wait between
// steps, recordable, and the per-evaluator chain bit for bit.
//
// The walk's SCHEDULE -- which steps end a run of steps, where the widths are re-tuned, how a run splits into graph
// replays and a remainder, how many passes a round of the look-ahead walk launches,
// which form the steps take (choose_form) -- is walk_plan.h: pure functions, tested without a device.  The walk and
// LockstepSet::launch call them and hold no copy of those rules.
//
// The walk's STRUCTURE: MCMC::operator() sets up, chooses the form, walks run by run and finishes, over a Walk object
// (private to MCMC) that holds the walk's arrays, its one argument block, its graph, its stream and the set-up lock;
// every part is a member of Walk that says which lock it needs.  ~Walk is the scope guard: on every way out the
// evaluators are un-bound from the arrays, the lockstep set is left and graph and stream are released under the lock,
// before the arrays die.  Handles are owned (Owned<>); record_graph is the one recorder of launches into a graph.
#pragma once

#include <limits>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "chain.h"
#include "fit_types.h"
#include "nll_kernels.h"
#include "walk_plan.h"

namespace sxmc {

/** The lock that serialises set-up, graph recording and tear-down of the chains that share a DEVICE (allocation,
 *  uploads through the legacy stream, launch-plan rebuilds and device-wide synchronisation are calls the runtime
 *  refuses, or stalls, beside another thread's recording on that device).  A std::mutex that also keeps the time its
 *  users spent waiting for it and holding it: with G devices x lanes host threads that is the Amdahl term of an
 *  ensemble, and a run reports it instead of guessing (bench_cpp: "setup_lock").  One per device: chains on
 *  different devices never contend. */
/** Shared by the SetupLocks of several cards (ensemble_multi_gpu with one lock per card): GRAPH RECORDING anywhere in the
 *  process excludes set-up -- allocation, uploads, launch plans, module loads, device-wide synchronisation --
 *  everywhere in the process, while the set-ups of different cards run side by side.  Holding a SetupLock holds the gate
 *  shared; begin_recording() trades that for the exclusive side until end_recording(). */
struct RecordingGate {
  std::shared_timed_mutex m;
};

class SetupLock {
 public:
  SetupLock() = default;
  explicit SetupLock(RecordingGate* gate_) : gate(gate_) {}
  void lock() {
    const auto t0 = std::chrono::steady_clock::now();
    m.lock();
    if (gate) gate->m.lock_shared();
    since = std::chrono::steady_clock::now();
    waited_ns.fetch_add((unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(since - t0).count(),
                        std::memory_order_relaxed);
    acquisitions.fetch_add(1, std::memory_order_relaxed);
  }
  void unlock() {
    held_ns.fetch_add((unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - since).count(),
                      std::memory_order_relaxed);
    if (gate) gate->m.unlock_shared();
    m.unlock();
  }
  /** The holder is about to record a HIP graph: nobody in the process may be inside a set-up section meanwhile (the
   *  other holders of the gate finish theirs first; new ones wait).  Only the holder of this lock calls these. */
  void begin_recording() {
    if (!gate) return;
    gate->m.unlock_shared();
    gate->m.lock();
  }
  void end_recording() {
    if (!gate) return;
    gate->m.unlock();
    gate->m.lock_shared();
  }
  double waited_seconds() const { return 1e-9 * (double)waited_ns.load(); }   //!< summed over all the threads that asked
  double held_seconds() const { return 1e-9 * (double)held_ns.load(); }
  unsigned long long count() const { return acquisitions.load(); }

 private:
  std::mutex m;
  RecordingGate* gate = nullptr;
  std::chrono::steady_clock::time_point since;   // (written and read by the holder only)
  std::atomic<unsigned long long> waited_ns{0}, held_ns{0}, acquisitions{0};
};

/** begin_recording / end_recording of a held SetupLock (may be null or not held: nothing to do then), scope-bound. */
struct RecordingScope {
  SetupLock* lock;
  explicit RecordingScope(SetupLock* l, bool held) : lock(held ? l : nullptr) {
    if (lock) lock->begin_recording();
  }
  ~RecordingScope() {
    if (lock) lock->end_recording();
  }
  RecordingScope(const RecordingScope&) = delete;
  RecordingScope& operator=(const RecordingScope&) = delete;
};

/** A library handle that is destroyed with its owner: move-only.  reset() passes the library's answer on. */
template <typename H, int (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  explicit Owned(H h_) : h(h_) {}
  ~Owned() { reset(); }
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h = o.h;
      o.h = nullptr;
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  int reset() {
    const int rc = h ? Destroy(h) : SXMC_OK;
    h = nullptr;
    return rc;
  }
  H get() const { return h; }
  H* put() {   //!< for a `create(..., &out)` call: what was owned goes first
    reset();
    return &h;
  }
  explicit operator bool() const { return h != nullptr; }

 private:
  H h = nullptr;
};
typedef Owned<sxmc_graph_t, sxmc_graph_destroy> OwnedGraph;
typedef Owned<sxmc_multigroup_t, sxmc_multigroup_destroy> OwnedMultigroup;
typedef Owned<sxmc_group_t, sxmc_group_destroy> OwnedGroup;
typedef Owned<sxmc_stream_t, sxmc_stream_destroy> OwnedStream;   //!< a stream its holder created itself

/** Records n calls of launch_one (which returns the library's rc, or throws) on `stream` into `graph`, replacing what
 *  it held.  `lock`, when `held`, trades its side of the recording gate for the exclusive one meanwhile.  The capture is
 *  ALWAYS ended; after a failure the partial graph is destroyed, `graph` is empty, and the FIRST error is what comes
 *  back: as the rc, with its text in *why when given (ending the capture may fail in turn and overwrite the library's
 *  last error), or as launch_one's exception. */
template <typename F>
int record_graph(sxmc_stream_t stream, SetupLock* lock, bool held, unsigned n, OwnedGraph& graph, F&& launch_one,
                 std::string* why = nullptr) {
  RecordingScope recording(lock, held);
  graph.reset();
  int rc = sxmc_graph_begin_capture(stream);
  if (rc) {
    if (why) *why = sxmc_last_error();
    return rc;
  }
  auto end = [&]() {
    sxmc_graph_t recorded = nullptr;
    const int rc2 = sxmc_graph_end_capture(stream, &recorded);
    graph = OwnedGraph(recorded);
    return rc2;
  };
  try {
    for (unsigned k = 0; k < n && rc == SXMC_OK; k++) rc = launch_one();
  } catch (...) {
    end();
    graph.reset();
    throw;
  }
  if (rc && why) *why = sxmc_last_error();
  const int rc2 = end();
  if (rc == SXMC_OK && rc2 && why) *why = sxmc_last_error();
  if (rc || rc2) graph.reset();
  return rc ? rc : rc2;
}

/** Chains advanced TOGETHER (sxmc_multigroup_step_async): one fill pass over the shared sample tables per step for
 *  all of them, then every chain's own step end.  Shared by the MCMC objects of one lockstep set, each walking on
 *  its own host thread and on the set's ONE stream: a chain that is ready for its next run of steps leaves its
 *  arguments here; the last one to arrive launches the run for all -- replays of a HIP graph of `graph_steps`
 *  recorded lockstep steps, the remainder step by step -- so the host threads meet once per run (a handful of
 *  times per walk), not once per step.  Every chain of the set must ask for the same runs. */
class LockstepSet {
 public:
  /** exclusive: the mutex that serialises set-up, graph recording and tear-down in this process (may be null). */
  LockstepSet(size_t nchains, sxmc_stream_t stream_, SetupLock* exclusive_ = nullptr)
      : stream(stream_), exclusive(exclusive_), groups(nchains, nullptr), args(nchains) {}
  LockstepSet(const LockstepSet&) = delete;
  LockstepSet& operator=(const LockstepSet&) = delete;

  /** Chain `index` is ready to take `nsteps` steps with `a`: returns when those steps of ALL chains are launched. */
  void advance(size_t index, sxmc_group_t group, const sxmc_step_args& a, unsigned nsteps, unsigned graph_steps) {
    std::unique_lock<std::mutex> lock(m);
    if (broken) throw std::runtime_error("lockstep set: " + why);
    if (groups[index] != group || std::memcmp(&args[index], &a, sizeof a) != 0) dirty = true;
    groups[index] = group;
    args[index] = a;
    const unsigned long long gen = generation;
    if (++arrived == groups.size()) {
      int rc = launch(nsteps, graph_steps);
      arrived = 0;
      generation++;
      if (rc != SXMC_OK) {
        broken = true;
        if (why.empty()) why = sxmc_last_error();   // (a failed recording has left its first error there)
      }
      cv.notify_all();
      if (broken) throw std::runtime_error("lockstep set: " + why);
    } else {
      cv.wait(lock, [&] { return generation != gen || broken; });
      if (broken) throw std::runtime_error("lockstep set: " + why);
    }
  }
  /** The chain's group is about to be destroyed: multigroup and graph are rebuilt at the next run. */
  void leave(size_t index) {
    std::lock_guard<std::mutex> lock(m);
    groups[index] = nullptr;
    dirty = true;
  }
  /** A chain of the set failed: its partners must not wait for it. */
  void abandon(const std::string& reason) {
    std::lock_guard<std::mutex> lock(m);
    broken = true;
    why = reason;
    cv.notify_all();
  }
  sxmc_stream_t stream;

 private:
  int launch(unsigned nsteps, unsigned graph_steps) {
    if (dirty) {
      graph.reset();
      int rc = sxmc_multigroup_create(groups.data(), (int)groups.size(), mg.put());
      if (rc) return rc;
      dirty = false;
      stepped = false;
    }
    const RunSplit run = split_run(nsteps, graph_steps, !stepped);
    if (run.replays > 0) {
      if (!graph || recorded != graph_steps) {
        // recording does not tolerate another thread's allocations: under the process's set-up mutex
        std::unique_lock<SetupLock> excl;
        if (exclusive) excl = std::unique_lock<SetupLock>(*exclusive);
        int rc = record_graph(stream, exclusive, exclusive != nullptr, graph_steps, graph,
                              [&]() { return sxmc_multigroup_step_async(mg.get(), stream, args.data()); }, &why);
        if (rc) return rc;
        recorded = graph_steps;
      }
      int rc = sxmc_graph_launch(graph.get(), stream, (int)run.replays);
      if (rc) return rc;
      nsteps = run.remainder;
    }
    for (unsigned k = 0; k < nsteps; k++) {
      // the first step of a new set of chains builds launch plans (allocations, a device-wide synchronisation),
      // which another set's recording does not tolerate: under the process's set-up mutex, like the recording
      std::unique_lock<SetupLock> excl;
      if (!stepped && exclusive) excl = std::unique_lock<SetupLock>(*exclusive);
      int rc = sxmc_multigroup_step_async(mg.get(), stream, args.data());
      if (rc) return rc;
      stepped = true;   // (the launch plans are in place once a step has been launched: recording may follow)
    }
    return SXMC_OK;
  }

  std::mutex m;
  std::condition_variable cv;
  SetupLock* exclusive;
  std::vector<sxmc_group_t> groups;
  std::vector<sxmc_step_args> args;
  OwnedMultigroup mg;   // (declared before the graph recorded over it: destroyed after it)
  OwnedGraph graph;
  unsigned recorded = 0;
  size_t arrived = 0;
  unsigned long long generation = 0;
  bool dirty = true, broken = false, stepped = false;
  std::string why;
};

/** The proposal of a walk: the reference's independent Gaussians, or v_current + L z with L rebuilt at the two
 *  re-tunings from the chain's own correlations (README, "Correlated proposals"). */
enum class Proposal { DIAGONAL, COVARIANCE };

class MCMC {
 public:
  Proposal proposal = Proposal::DIAGONAL;   //!< COVARIANCE: the next proposal is v_current + L z, L the lower-triangular
                                            //!< factor sxmc_proposal_factor builds at each re-tuning (diag(w) before the
                                            //!< first); every marginal width stays the reference's.  Every sequential
                                            //!< form takes it; asked with lookahead the walk goes sequentially; a chain
                                            //!< of a lockstep set refuses it
  double proposal_shrinkage = 0.05;         //!< in (0, 1]: the correlations are shrunk towards the identity by this much
  std::vector<double> constraint_correlation;   //!< empty: one independent Gaussian constraint per parameter.  Otherwise
                                            //!< P x P, a correlation matrix over the parameter vector (sources, then the
                                            //!< systematics' parameters) that ties the constraints together: the NLL's
                                            //!< constraint terms become 0.5 r_i^2 of the whitened residuals r = W x
                                            //!< (README, "Correlated constraints"; sxmc_constraint_whitening validates and
                                            //!< whitens).  Every sequential form takes it; asked with lookahead the walk
                                            //!< goes sequentially; a chain of a lockstep set refuses it
  LockstepSet* lockstep = nullptr;  //!< set: this chain steps together with the other chains of the set (same
  size_t lockstep_index = 0;        //!< sample tables, same systematics, the set's stream); every run of steps is
                                    //!< launched (graph replays of graph_steps steps) by the chain that arrives last
  bool reference_form = false;  //!< launch the reference's own kernel sequence instead of the batched one
  bool verbose = false;
  unsigned graph_steps = 0;     //!< > 0: replay the batched step from a HIP graph of this many recorded steps
  bool optimize = true;         //!< EvalHist's `optimize` constructor flag for the batched launch: a few trial
                                //!< launches at the start of a walk pick the lane count per CU (sxmc_group_optimize)
  bool consume = true;          //!< batched form: the step end also clears histograms and normalisations for the
                                //!< next step (sxmc_group_step_async: 2 launches per step; nothing reads them
                                //!< between the steps of a walk)
  SetupLock* exclusive = nullptr;   //!< with one chain per host thread: the lock this walk holds while it
                                    //!< allocates, uploads, rebuilds launch plans, records its graph and frees
                                    //!< (calls the runtime refuses beside another thread's recording); it is
                                    //!< released while the walk only launches and waits on its own stream
  bool lookahead = false;       //!< batched, consuming form, one chain: the LOOK-AHEAD WALK.  Every pass over the tables
                                //!< evaluates the step's proposal AND the vector the next step proposes after a rejection
                                //!< (a second set of evaluators over the same tables), and the step end decides one or two
                                //!< steps (sxmc_multigroup_lookahead_step_async).  Same chain bit for bit; +25 % steps
                                //!< per second where the fill streams float columns (it is bound by the stream, and the
                                //!< pass streams once for two evaluations), SLOWER where it streams 16-bit codes (the
                                //!< pass is then bound by its arithmetic: BASELINE config 3, 9 380 against 10 290).
  unsigned adapt_interval = 1000;  //!< a plan with two forms of the fill: steps between the flushes at which the walk asks
                                   //!< which one to take (sxmc_group_adapt_fill_form); 0: only at the reference's flushes
  bool lookahead_auto = false;  //!< let the walk decide: the look-ahead pass where the launch plan streams float columns,
                                //!< one evaluation per step where it streams codes (what the measurements above say)
  /** Hooks for a driver that runs several walks side by side (sxmc::ensemble_concurrent): called once the walk's
   *  set-up is over -- buffers, first evaluation, launch plan, recorded graph; the set-up lock released -- and BEFORE
   *  its first long run of steps is queued; and once its last step has finished, before its tear-down.  An ensemble's
   *  lanes meet at both: set-up and tear-down synchronise the whole device (allocation, launch plans), and beside a
   *  chain that has a second of replays queued every one of those calls waits that second out -- measured at 1e5
   *  steps per experiment: eight lanes walked ONE AT A TIME, 10 500 steps/s for the card (profiles/r05_c4_lanes.log). */
  std::function<void()> on_setup_done, on_steps_done;
  bool lut_output = false;      //!< materialise the lookup table in the batched step (nothing reads it; when
                                //!< false the event sum runs over distinct event-bin tuples, see sxmc_hip.h)
  bool columns_in_place = false;  //!< MIXED form: sum the events with the histogram columns looked up in place
                                  //!< (sxmc_group_eval_columns_nll_async: one launch less, the members' columns of the
                                  //!< table not written) instead of materialising them.  Same chain bit for bit.  Off
                                  //!< by default: measured 0.8-1.4 % SLOWER per step at 8 histogram signals x
                                  //!< 4.75e4 events (its look-ups and divisions sit on the event sum's 64
                                  //!< workgroups), 4 % faster at 1 x 874 (README, "Mixed walks"); ignored with
                                  //!< lut_output
  unsigned long long seed = 0;  //!< gRandom->GetSeed() in the reference (mcmc.cpp:125)

  MCMC(const std::vector<Source>& sources, const std::vector<Signal>& signals,
       const std::vector<Systematic>& systematics, const std::vector<Observable>& observables,
       unsigned long long _seed = 1, sxmc_stream_t _stream = nullptr)
      : seed(_seed),
        stream(_stream),
        nsources(sources.size()),
        nsignals(signals.size()),
        nsystematics(systematics.size()),
        nobservables(observables.size()) {
    // mcmc.cpp:37-45: launch shapes of the NLL kernels
    nnllblocks = 64;
    nllblocksize = 256;
    nnllthreads = nnllblocks * nllblocksize;
    nreducethreads = 128;

    size_t npars = 0;
    for (const Systematic& s : systematics) npars += s.npars;
    nparameters = nsources + npars;
    parameter_means.reset(new pdfz::Array<double>(nparameters, true));
    parameter_sigma.reset(new pdfz::Array<double>(nparameters, true));
    parameter_fixed.resize(nparameters);
    nfloat = 0;
    for (size_t i = 0; i < nsources; i++) {
      parameter_means->writeOnlyHostPtr()[i] = sources[i].mean;
      parameter_sigma->writeOnlyHostPtr()[i] = sources[i].sigma;
      parameter_fixed[i] = sources[i].fixed;
      nfloat += sources[i].fixed ? 0 : 1;
      parameter_names.push_back(sources[i].name);
    }
    systematics_fixed = true;
    size_t k = nsources;
    for (const Systematic& s : systematics) {
      if (!s.fixed) systematics_fixed = false;
      for (size_t j = 0; j < s.npars; j++) {
        parameter_means->writeOnlyHostPtr()[k] = s.means[j];
        parameter_sigma->writeOnlyHostPtr()[k] = s.sigmas[j];
        parameter_fixed[k] = s.fixed;
        nfloat += s.fixed ? 0 : 1;
        parameter_names.push_back(s.name + "_" + std::to_string(j));
        k++;
      }
    }
    parameter_names.push_back("likelihood");

    nexpected.reset(new pdfz::Array<double>(nsignals, true));
    n_mc.reset(new pdfz::Array<unsigned>(nsignals, true));
    source_id.reset(new pdfz::Array<short>(nsignals, true));
    for (size_t i = 0; i < nsignals; i++) {
      pdfs.push_back(signals[i].histogram);
      nexpected->writeOnlyHostPtr()[i] = signals[i].nexpected;
      n_mc->writeOnlyHostPtr()[i] = (unsigned)signals[i].n_mc;
      source_id->writeOnlyHostPtr()[i] = (short)signals[i].source.index;
    }

    rngs.reset(new pdfz::Array<RNGState>(nparameters, true));
    const int bs = 128;
    const int nb = (int)(nparameters / bs + 1);
    SXMC_KERNEL_LAUNCH(init_device_rngs, nb, bs, 0, stream, (int)nparameters, seed, rngs->writeOnlyPtr());

    // the batched forms need every evaluator to be a histogram evaluator of this library; with kernel-density
    // evaluators of this library among them the walk is MIXED: the histogram members form the group (none: no group),
    // which is told where its members' columns sit among the signals'
    std::vector<sxmc_hist_t> handles;
    std::vector<int> member_of_signal;
    for (pdfz::Eval* p : pdfs) {
      pdfz::EvalHist* h = dynamic_cast<pdfz::EvalHist*>(p);
      pdfz::EvalKernel* k = dynamic_cast<pdfz::EvalKernel*>(p);
      if (!h && !k) {
        handles.clear();
        kernels.clear();
        break;
      }
      member_of_signal.push_back(h ? (int)handles.size() : -1);
      if (h) handles.push_back(h->Handle());
      if (k) kernels.push_back(KernelMember{k, false});
    }
    if (!handles.empty()) check(sxmc_group_create(handles.data(), (int)handles.size(), &group));
    if (group && !kernels.empty()) {
      const int rc = sxmc_group_set_columns(group, (int)member_of_signal.size(), member_of_signal.data());
      if (rc) {
        sxmc_group_destroy(group);   // (the destructor does not run for an object whose constructor threw)
        group = nullptr;
        check(rc);
      }
    }
  }

  ~MCMC() {
    if (group) sxmc_group_destroy(group);
  }
  MCMC(const MCMC&) = delete;
  MCMC& operator=(const MCMC&) = delete;

  /** Initial proposal widths, mcmc.cpp:198-228 (including its `i < nsignals` test at :217). */
  std::vector<float> initial_jump_widths() const {
    std::vector<float> w(nparameters);
    const float scale_factor = 2.4 * 2.4 / nfloat;  // Haario, 2001
    for (size_t i = 0; i < nparameters; i++) {
      if (parameter_fixed[i]) {
        w[i] = -1;
        continue;
      }
      const float mean = parameter_means->readOnlyHostPtr()[i];
      const float sigma = parameter_sigma->readOnlyHostPtr()[i];
      float width = 0.1;
      if (sigma > 0) {
        width = sigma;
      } else if (i < nsignals) {
        const float m = std::max(mean, (float)10);
        width = std::sqrt(m) / m;
      } else {
        width = std::sqrt(std::max(mean, (float)1));
      }
      w[i] = 0.1 * width * scale_factor;
    }
    return w;
  }

  /** MCMC::operator() (mcmc.cpp:143-387).  data: rows of nobservables+1 floats (last = dataset id).
   *  Set up, choose the form of the steps, walk run by run, tear down: the parts are the members of Walk below. */
  Chain operator()(std::vector<float>& data, unsigned nsteps, float burnin_fraction,
                   const bool debug_mode = false, unsigned sync_interval = 10000) {
    return walk(data, nullptr, nsteps, burnin_fraction, debug_mode, sync_interval);
  }
  /** The same over WEIGHTED data events: event_weights[i], a finite double >= 0, is row i's weight in the likelihood's
   *  event term, sum_i w_i log(s_i) (include/sxmc_hip.h, sxmc_group_set_event_weights: the law).  Every sequential form
   *  takes them -- reference_form and the MIXED form through sxmc_launch_nll_event_chunks_weighted over the whole table,
   *  the batched and consuming forms through the group; asked with lookahead the walk goes sequentially.  Refused, with
   *  pdfz::Error: a weight that is not finite and >= 0, a count that is not the data's, columns_in_place, a chain of a
   *  lockstep set. */
  Chain operator()(std::vector<float>& data, const std::vector<double>& event_weights, unsigned nsteps,
                   float burnin_fraction, const bool debug_mode = false, unsigned sync_interval = 10000) {
    return walk(data, &event_weights, nsteps, burnin_fraction, debug_mode, sync_interval);
  }

 protected:
  Chain walk(std::vector<float>& data, const std::vector<double>* event_weights, unsigned nsteps, float burnin_fraction,
             const bool debug_mode, unsigned sync_interval) {
    const std::chrono::steady_clock::time_point walk_t0 = std::chrono::steady_clock::now();
    Walk w(*this, data, event_weights, nsteps, burnin_fraction, debug_mode, sync_interval);
    w.set_up();
    w.choose_form();
    const std::chrono::steady_clock::time_point steps_t0 = std::chrono::steady_clock::now();
    w.chain.setup_seconds = std::chrono::duration<double>(steps_t0 - walk_t0).count();
    for (unsigned i = 0; i < nsteps;) i = w.run(i);
    return w.finish(steps_t0);
  }

 public:
  size_t NumParameters() const { return nparameters; }
  /** The factor the last walk ended with, P x P doubles with L_ij at [j * P + i] (empty after a DIAGONAL walk), and
   *  the shrinkage it was built with (doubled where a pivot failed: sxmc_proposal_factor). */
  const std::vector<double>& ProposalFactor(double* shrinkage_used = nullptr) const {
    if (shrinkage_used) *shrinkage_used = last_shrinkage;
    return last_factor;
  }
  /** The whitening matrix the last walk's constraints went through, P x P doubles with W_ij at [j * P + i]; empty
   *  after a walk without constraint_correlation. */
  const std::vector<double>& ConstraintWhitening() const { return last_whitening; }
  /** The form the steps of the last walk took (walk_plan.h: WalkForm::Step), valid after a walk: "reference", "batched",
   *  "consuming", "lockstep", "lookahead" or "mixed". */
  const char* WalkFormName() const { return form_name; }
  /** Look-ahead walk: passes over the tables launched so far (each evaluates twice and takes one or two steps). */
  size_t LookaheadPasses() const { return ahead_passes; }

  /** The launch plan of the chain's group as the library describes it (sxmc_group_launch_info): which table form and
   *  kernel each launch of the fill takes.  Empty when the walk is not batched. */
  std::string LaunchPlan() const {
    if (!group) return std::string();
    char buf[2048];
    buf[0] = 0;
    if (sxmc_group_launch_info(group, buf, sizeof buf) != SXMC_OK) return std::string();
    return std::string(buf);
  }

 protected:
  /** nll_event_chunks over the whole table in the reference's launch shape; weights (device, one per event): the
   *  weighted launch point. */
  void event_chunks(sxmc_stream_t s, const float* lut, size_t nevents, const double* v, const double* d_nexpected,
                    const unsigned* d_n_mc, const short* d_source_id, const unsigned* norms, double* sums,
                    const double* weights) {
    if (weights) {
      SXMC_KERNEL_LAUNCH(nll_event_chunks_weighted, nnllblocks, nllblocksize, 0, s, lut, v, nevents, nsignals,
                         d_nexpected, d_n_mc, d_source_id, norms, sums, weights);
    } else {
      SXMC_KERNEL_LAUNCH(nll_event_chunks, nnllblocks, nllblocksize, 0, s, lut, v, nevents, nsignals, d_nexpected, d_n_mc,
                         d_source_id, norms, sums);
    }
  }

  /** MCMC::nll (mcmc.cpp:390-415): three launches over an evaluated lookup table. */
  void nll(const float* lut, size_t nevents, const double* v, double* out, const unsigned* norms,
           double* event_partial_sums, double* event_total_sum, const double* weights = nullptr,
           const double* whitening = nullptr) {
    event_chunks(stream, lut, nevents, v, nexpected->readOnlyPtr(), n_mc->readOnlyPtr(), source_id->readOnlyPtr(), norms,
                 event_partial_sums, weights);
    SXMC_KERNEL_LAUNCH(nll_event_reduce, 1, nreducethreads, nreducethreads * sizeof(double), stream,
                       (size_t)nnllthreads, event_partial_sums, event_total_sum);
    SXMC_KERNEL_LAUNCH(nll_total, 1, 1, 0, stream, nparameters, v, nsignals, nsources,
                       parameter_means->readOnlyPtr(), parameter_sigma->readOnlyPtr(), event_total_sum,
                       nexpected->readOnlyPtr(), n_mc->readOnlyPtr(), source_id->readOnlyPtr(), norms, out, whitening);
  }

  static double column_stddev(const Chain& c, size_t col) {
    const size_t n = c.nrows();
    if (n < 2) return 0.0;
    double s = 0, s2 = 0;
    for (size_t r = 0; r < n; r++) {
      const double x = c.at(r, col);
      s += x;
      s2 += x * x;
    }
    const double var = s2 / n - (s / n) * (s / n);
    return var > 0 ? std::sqrt(var) : 0.0;
  }

 private:
  /** The arguments of a step: the library's block plus the two pointers it lacks.  Zeroed once, padding included (a
   *  LockstepSet compares blocks bytewise), and filled once per run (Walk::resolve). */
  struct StepArgs {
    sxmc_step_args a;
    const float* lut;
    double* sums;
  };

  /** The look-ahead walk's second set of evaluators over the same tables, bound to the look-ahead vector, and the pair
   *  it forms with the chain's own group.  Members die in reverse order: the pair before its groups, the group before
   *  its evaluators, the evaluators before the arrays they borrowed. */
  struct Shadow {
    Shadow(size_t nparameters, size_t nsignals, size_t nevents)
        : vector(nparameters, true), norms(nsignals, true), lut(nevents * nsignals, true), stop(1, true) {}
    pdfz::Array<double> vector;
    pdfz::Array<unsigned> norms;
    pdfz::Array<float> lut;
    pdfz::Array<int> stop;
    std::vector<std::unique_ptr<pdfz::EvalHist>> evaluators;
    OwnedGroup group;
    OwnedMultigroup pair;
    bool planned = false;   //!< the pair has launched once: its launch plans exist
  };

  /** array transfers of a walk are ordered on the chain's stream (a blocking copy through the legacy default stream
   *  would neither wait for a non-blocking stream nor leave other chains alone) */
  struct TransferGuard {
    sxmc_stream_t prev;
    explicit TransferGuard(sxmc_stream_t s) : prev(transfer_stream()) {
      if (s) transfer_stream() = s;
    }
    ~TransferGuard() { transfer_stream() = prev; }
  };

  /** One walk of the chain: its arrays, its graph, its stream, and the set-up lock it holds or has dropped.  THE LOCK IS
   *  THE FIRST MEMBER: it is released last, after every array below is freed.  ~Walk is the walk's scope guard: its body
   *  runs before any member dies, on the normal path (finish() has torn down then) and when a check() or a hook of the
   *  caller's threw -- then it tears down with errors swallowed, and the exception travels on. */
  struct Walk {
    MCMC& m;
    std::unique_lock<SetupLock> excl;
    TransferGuard transfer_guard;
    std::vector<float>& data;
    const bool debug_mode;
    const WalkSchedule plan;   // which steps end a run and where the widths are re-tuned: walk_plan.h
    const size_t ncol, nevents;
    const float scale_factor;
    Chain chain;
    pdfz::Array<double> current_vector, proposed_vector;
    pdfz::Array<unsigned> normalizations;
    pdfz::Array<double> event_partial_sums, event_total_sum;
    pdfz::Array<int> jump_counter, accept_counter;
    pdfz::Array<float> jump_buffer;
    pdfz::Array<double> current_nll, proposed_nll;
    pdfz::Array<float> jump_width, lut;
    const std::vector<double>* const event_weights;   // the data's weights, one per event, or null
    std::unique_ptr<pdfz::Array<double>> weights;     // ... on the device, for the weighted launch point
    const bool covariance;            // the walk's proposal is the correlated one
    std::unique_ptr<pdfz::Array<double>> factor;   // its factor, P x P: one device array for the walk's lifetime (none otherwise)
    const bool constrained;           // the walk's constraints are correlated
    std::unique_ptr<pdfz::Array<double>> whitening;   // their whitening matrix, P x P, on the device (none otherwise)
    std::unique_ptr<Shadow> shadow;   // look-ahead walk only
    OwnedGraph graph;
    OwnedStream own_stream;           // recorded steps need a created stream: the walk's own when it was given none
    sxmc_stream_t strm;
    WalkForm form{};
    StepArgs d;
    const double* d_factor = nullptr; // the factor on the device, or null: resolved with d
    const double* d_weights = nullptr; // the event weights on the device, or null: resolved with d
    const double* d_whitening = nullptr; // the constraints' whitening matrix on the device, or null: resolved with d
    bool two_forms = false;           // the plan holds a boxed and an ordered form of the fill (asked at every run)
    bool setup_announced = false;     // on_setup_done has been called
    bool torn_down = false;

    Walk(MCMC& m_, std::vector<float>& data_, const std::vector<double>* event_weights_, unsigned nsteps,
         float burnin_fraction, bool debug_mode_, unsigned sync_interval)
        : m(m_),
          excl(m_.exclusive ? std::unique_lock<SetupLock>(*m_.exclusive) : std::unique_lock<SetupLock>()),
          transfer_guard(m_.stream),
          data(data_),
          debug_mode(debug_mode_),
          plan{nsteps, (unsigned)(nsteps * burnin_fraction), sync_interval, m_.adapt_interval},
          ncol(m_.nparameters + 1),
          nevents(data_.size() / (m_.nobservables + 1)),
          scale_factor(2.4 * 2.4 / m_.nfloat),
          current_vector(m_.nparameters, true),
          proposed_vector(m_.nparameters, true),
          normalizations(m_.nsignals, true),
          event_partial_sums(std::max<size_t>(m_.nnllthreads, 1024), true),
          event_total_sum(1, true),
          jump_counter(1, true),
          accept_counter(1, true),
          jump_buffer((size_t)sync_interval * ncol, true),
          current_nll(1, true),
          proposed_nll(1, true),
          jump_width(m_.nparameters, true),
          lut(nevents * m_.nsignals, true),
          event_weights(event_weights_),
          covariance(m_.proposal == Proposal::COVARIANCE),
          factor(covariance ? new pdfz::Array<double>(m_.nparameters * m_.nparameters, true) : nullptr),
          constrained(!m_.constraint_correlation.empty()),
          whitening(constrained ? new pdfz::Array<double>(m_.nparameters * m_.nparameters, true) : nullptr),
          strm(m_.stream) {
      std::memset(&d, 0, sizeof d);
      chain.names = m.parameter_names;
    }
    ~Walk() {
      if (torn_down) return;
      try {
        tear_down(true);
      } catch (...) {   // (the walk has failed already: its own exception is the one to report)
      }
    }
    Walk(const Walk&) = delete;
    Walk& operator=(const Walk&) = delete;

    /** Buffers, bindings and the first evaluation (mcmc.cpp:198-242).  Set-up lock: held throughout. */
    void set_up() {
      for (size_t i = 0; i < m.nparameters; i++)
        current_vector.writeOnlyHostPtr()[i] = m.parameter_means->readOnlyHostPtr()[i];
      proposed_vector.writeOnlyHostPtr();
      normalizations.writeOnlyHostPtr();
      event_partial_sums.writeOnlyHostPtr();
      event_total_sum.writeOnlyHostPtr();
      jump_counter.writeOnlyHostPtr()[0] = 0;
      accept_counter.writeOnlyHostPtr()[0] = 0;
      current_nll.writeOnlyHostPtr();
      proposed_nll.writeOnlyHostPtr();
      const std::vector<float> w = m.initial_jump_widths();
      for (size_t i = 0; i < m.nparameters; i++) jump_width.writeOnlyHostPtr()[i] = w[i];
      m.last_factor.clear();
      if (covariance) {
        if (m.lockstep) throw pdfz::Error("MCMC: a lockstep set has no correlated step end: walk a COVARIANCE chain alone");
        rebuild_factor(nullptr, 0);   // (L = diag(w), through the re-tuning's own code)
      }
      m.last_whitening.clear();
      if (constrained) {
        if (m.constraint_correlation.size() != m.nparameters * m.nparameters) {
          throw pdfz::Error("MCMC: constraint_correlation holds " + std::to_string(m.constraint_correlation.size()) +
                            " entries for " + std::to_string(m.nparameters) + " x " + std::to_string(m.nparameters));
        }
        if (m.lockstep) {
          throw pdfz::Error("MCMC: a lockstep set has no step end with correlated constraints: walk a chain with a "
                            "constraint_correlation alone");
        }
        // (validated and whitened by the library's one implementation; a refusal names the entry or the pivot)
        check(sxmc_constraint_whitening(m.constraint_correlation.data(), m.parameter_sigma->readOnlyHostPtr(),
                                        (int)m.nparameters, whitening->writeOnlyHostPtr()));
        m.last_whitening.assign(whitening->readOnlyHostPtr(), whitening->readOnlyHostPtr() + m.nparameters * m.nparameters);
      }
      if (event_weights) {
        if (event_weights->size() != nevents) {
          throw pdfz::Error("MCMC: " + std::to_string(event_weights->size()) + " event weights for " +
                            std::to_string(nevents) + " events");
        }
        for (size_t i = 0; i < nevents; i++) {   // (the group checks its copy too; a walk without a group has only this)
          const double w = (*event_weights)[i];
          if (!(w >= 0.0) || w > std::numeric_limits<double>::max()) {
            throw pdfz::Error("MCMC: event weight " + std::to_string(i) + " is not a finite number >= 0");
          }
        }
        if (m.lockstep) throw pdfz::Error("MCMC: a lockstep set has no weighted step end: walk a chain over weighted events alone");

        if (m.columns_in_place) {
          throw pdfz::Error("MCMC: columns_in_place has no weighted event sum: walk weighted events with the table materialised");
        }
        weights.reset(new pdfz::Array<double>(std::max<size_t>(nevents, 1), true));
        for (size_t i = 0; i < nevents; i++) weights->writeOnlyHostPtr()[i] = (*event_weights)[i];
      }
      // (the group keeps a copy for its own event sums: this walk's, or none -- refuses what is not finite and >= 0)
      if (m.group) check(sxmc_group_set_event_weights(m.group, event_weights ? event_weights->data() : nullptr, event_weights ? nevents : 0));

      // mcmc.cpp:230-242: bind, first evaluation at the current vector, then re-point at the proposal
      for (size_t i = 0; i < m.pdfs.size(); i++) {
        pdfz::Eval* p = m.pdfs[i];
        p->SetEvalPoints(data);
        p->SetPDFValueBuffer(&lut, (int)(i * nevents), 1);
        p->SetNormalizationBuffer(&normalizations, (int)i);
        p->SetParameterBuffer(&current_vector, (int)m.nsources);
        p->EvalAsync();
        p->EvalFinished();
        p->SetParameterBuffer(&proposed_vector, (int)m.nsources);
      }
      m.nll(lut.readOnlyPtr(), nevents, current_vector.readOnlyPtr(), current_nll.writeOnlyPtr(),
            normalizations.readOnlyPtr(), event_partial_sums.ptr(), event_total_sum.ptr(),
            weights ? weights->readOnlyPtr() : nullptr, whitening ? whitening->readOnlyPtr() : nullptr);
      SXMC_KERNEL_LAUNCH(pick_new_vector, 1, 64, 0, m.stream, (int)m.nparameters, m.rngs->ptr(),
                         jump_width.readOnlyPtr(), current_vector.readOnlyPtr(), proposed_vector.writeOnlyPtr());
    }

    /** The form of the steps (walk_plan.h: choose_form), narrowed by what the device says about the look-ahead pass;
     *  then what the form needs: the group bound and tuned, the shadow set, a stream to record on.  Lock: held. */
    void choose_form() {
      // weighted Monte Carlo samples (EvalHist::SetSampleMultiplicities): only the fill differs, every sequential form
      // takes them; a lockstep set has no weighted fill and is refused by name, a walk asked with lookahead goes sequentially
      bool sample_weights = false;
      for (pdfz::Eval* p : m.pdfs)
        if (pdfz::EvalHist* h = dynamic_cast<pdfz::EvalHist*>(p)) sample_weights = sample_weights || h->HasSampleMultiplicities();
      if (sample_weights && m.lockstep) {
        throw pdfz::Error("MCMC: a lockstep set has no weighted fill: walk a chain over signals with sample multiplicities alone");
      }
      form = sxmc::choose_form(covariance, event_weights != nullptr, sample_weights, constrained,
                               WalkFlags{m.group != nullptr, m.reference_form,
                                         m.nsystematics > 0 && !m.systematics_fixed, m.consume, m.lut_output,
                                         m.lockstep != nullptr, m.lookahead || m.lookahead_auto, m.nparameters,
                                         m.graph_steps, !m.kernels.empty()});
      if (form.step == WalkForm::MIXED) {
        // the kernel members are launched through their handles: bindings current, and which of them a step re-evaluates
        for (KernelMember& k : m.kernels) {
          k.eval->Bind();
          short pars[SXMC_MAX_SYST * SXMC_MAX_SYST_PARS];
          size_t n = 0;
          check(sxmc_kde_parameters_read(k.eval->Handle(), pars, sizeof pars / sizeof pars[0], &n));
          if (n > sizeof pars / sizeof pars[0]) throw pdfz::Error("MCMC: a kernel-density signal reads too many parameters");
          k.floats = false;
          for (size_t q = 0; q < n; q++) {
            const size_t index = m.nsources + (size_t)pars[q];
            k.floats = k.floats || index >= m.nparameters || !m.parameter_fixed[index];
          }
        }
      }
      if (form.batched) {
        // bindings must be current before the group reads them (proposal vector as parameter buffer)
        for (pdfz::Eval* p : m.pdfs)
          if (pdfz::EvalHist* h = dynamic_cast<pdfz::EvalHist*>(p)) h->Bind();
        check(sxmc_group_set_lut_output(m.group, m.lut_output ? 1 : 0));
        if (m.optimize && !m.optimized) {
          check(sxmc_group_optimize(m.group, m.stream, nullptr));
          m.optimized = true;
        }
      }
      if (form.step == WalkForm::LOOKAHEAD && m.lookahead_auto && !m.lookahead) {
        int members = 0;
        unsigned long long rows = 0, exact_rows = 0, never_rows = 0;
        check(sxmc_group_codes_info(m.group, &members, &rows, &exact_rows, &never_rows));
        if (members != 0) form = form.narrowed();     // (a plan over codes walks sequentially)
      }
      if (form.step == WalkForm::LOOKAHEAD) {
        // not every shape is offered the look-ahead pass (histograms beyond LDS; problems so small that the sequential
        // step ends in the one-workgroup form, which the pass has no counterpart of): those walk sequentially
        int ok = 0;
        check(sxmc_group_lookahead_supported(m.group, &ok));
        if (!ok) form = form.narrowed();
      }
      if (form.step == WalkForm::LOOKAHEAD) set_up_shadow();
      // Recorded steps need a created stream (blocking: it still orders with the copies of the array accessors, which
      // go through the legacy default stream)
      if (form.gsteps > 0 && !strm) {
        check(sxmc_stream_create(own_stream.put()));
        strm = own_stream.get();
      }
      static const char* const names[] = {"reference", "batched", "consuming", "lockstep", "lookahead", "mixed"};
      m.form_name = names[form.step];
    }

    /** Look-ahead walk: a shadow set of evaluators over the same tables, bound to the look-ahead vector.  Lock: held. */
    void set_up_shadow() {
      shadow.reset(new Shadow(m.nparameters, m.nsignals, nevents));
      shadow->vector.writeOnlyHostPtr();
      shadow->norms.writeOnlyHostPtr();
      shadow->lut.writeOnlyHostPtr();
      std::vector<sxmc_hist_t> handles;
      for (size_t i = 0; i < m.pdfs.size(); i++) {
        pdfz::EvalHist* base = dynamic_cast<pdfz::EvalHist*>(m.pdfs[i]);
        shadow->evaluators.emplace_back(new pdfz::EvalHist(*base, pdfz::EvalHist::SharedSamples{}));
        pdfz::EvalHist* p = shadow->evaluators.back().get();
        p->SetEvalPoints(data);
        p->SetPDFValueBuffer(&shadow->lut, (int)(i * nevents), 1);
        p->SetNormalizationBuffer(&shadow->norms, (int)i);
        p->SetParameterBuffer(&shadow->vector, (int)m.nsources);
        p->Bind();
        handles.push_back(p->Handle());
      }
      check(sxmc_group_create(handles.data(), (int)handles.size(), shadow->group.put()));
      check(sxmc_group_set_lut_output(shadow->group.get(), 0));
      // a pass of two evaluations is bound by vector issue and needs more registers than 1024 lanes leave each
      // (spills inside the stream loop drain the loads in flight): 768 lanes, the kernel compiled for that bound
      check(sxmc_group_set_launch_config(m.group, 768, 1));
      check(sxmc_group_set_launch_config(shadow->group.get(), 768, 1));
      sxmc_group_t both[2] = {m.group, shadow->group.get()};
      check(sxmc_multigroup_create(both, 2, shadow->pair.put()));
    }

    /** Device pointers of one run of steps, resolved once per run: the accessors may copy (after the host wrote a
     *  counter or the widths), which must not happen while a graph is being recorded. */
    void resolve() {
      d.lut = lut.readOnlyPtr();
      d.sums = event_partial_sums.ptr();
      d.a.d_means = m.parameter_means->readOnlyPtr();
      d.a.d_sigmas = m.parameter_sigma->readOnlyPtr();
      d.a.d_rng = m.rngs->ptr();
      d.a.d_nll_current = current_nll.ptr();
      d.a.d_nll_proposed = proposed_nll.ptr();
      d.a.d_v_current = current_vector.ptr();
      d.a.d_v_proposed = proposed_vector.ptr();
      d.a.d_accepted = accept_counter.ptr();
      d.a.d_counter = jump_counter.ptr();
      d.a.d_jump_buffer = jump_buffer.writeOnlyPtr();
      d.a.nparameters = (int)m.nparameters;
      d.a.nsources = m.nsources;
      d.a.d_jump_width = jump_width.readOnlyPtr();
      d.a.d_nexpected = m.nexpected->readOnlyPtr();
      d.a.d_n_mc = m.n_mc->readOnlyPtr();
      d.a.d_source_id = m.source_id->readOnlyPtr();
      d.a.d_norms = normalizations.ptr();
      d.a.debug_mode = debug_mode ? 1 : 0;
      // the factor like the widths: uploaded here, after a re-tuning wrote it, never under a recording; the address is
      // the same for the whole walk, so recorded steps survive a re-tuning
      d_factor = covariance ? factor->readOnlyPtr() : nullptr;
      d_weights = weights ? weights->readOnlyPtr() : nullptr;
      d_whitening = whitening ? whitening->readOnlyPtr() : nullptr;
      if (m.group) check(sxmc_group_set_proposal_factor(m.group, d_factor));
      if (m.group) check(sxmc_group_set_constraint_whitening(m.group, d_whitening));
    }

    /** One step of the sequential walk, in the form's launches. */
    void one_step() {
      const sxmc_step_args& a = d.a;
      int npartial = (int)m.nnllthreads;
      if (form.step == WalkForm::MIXED) {
        mixed_step();
        return;
      }
      if (form.step == WalkForm::CONSUMING) {
        // two launches: fill of all signals; lookup + event sum + step end + clearing for the next step
        check(sxmc_group_step_async(m.group, strm, a.d_means, a.d_sigmas, a.d_rng, a.d_nll_current, a.d_nll_proposed,
                                    a.d_v_current, a.d_v_proposed, a.d_accepted, a.d_counter, a.d_jump_buffer,
                                    a.nparameters, a.nsources, a.d_jump_width, a.d_nexpected, a.d_n_mc, a.d_source_id,
                                    a.d_norms, a.debug_mode));
        return;
      }
      if (form.step == WalkForm::BATCHED) {
        // zero, fill of all signals in one kernel, lookup fused with the event partial sums
        check(sxmc_group_eval_nll_async(m.group, strm, a.d_v_proposed, a.d_nexpected, a.d_n_mc, a.d_source_id,
                                        a.d_norms, d.sums, &npartial));
      } else {
        if (form.reevaluate) {
          // mcmc.cpp:264-271 as written.  (The evaluators launch on their own streams, which order with the legacy
          // default stream -- where the reference launches its NLL kernels -- and with nothing else: a walk that was
          // given its own stream waits for its step end before the evaluators read the new proposal.)
          if (strm) check(sxmc_stream_synchronize(strm));
          for (pdfz::Eval* p : m.pdfs) p->EvalAsync();
          for (pdfz::Eval* p : m.pdfs) p->EvalFinished();
        }
        m.event_chunks(strm, d.lut, nevents, a.d_v_proposed, a.d_nexpected, a.d_n_mc, a.d_source_id, a.d_norms, d.sums,
                       d_weights);
      }
      SXMC_KERNEL_LAUNCH(finish_nll_jump_pick_combo, 1, m.nreducethreads, m.nreducethreads * sizeof(double), strm,
                         (size_t)npartial, d.sums, m.nsignals, m.nsources, a.d_means, a.d_sigmas, a.d_rng,
                         a.d_nll_current, a.d_nll_proposed, a.d_v_current, a.d_v_proposed, a.d_accepted, a.d_counter,
                         a.d_jump_buffer, a.nparameters, a.d_jump_width, a.d_nexpected, a.d_n_mc, a.d_source_id,
                         a.d_norms, debug_mode, d_factor, d_whitening);
    }

    /** One step of a MIXED walk, every launch on the walk's stream and none of them a wait, a copy or an allocation (so
     *  the step can be recorded): the kernel members that read a floating parameter (sxmc_kde_eval_on_stream_async), the
     *  group's evaluation into its columns of the table (sxmc_group_eval_async), nll_event_chunks over the whole table
     *  (the reference's 64 x 256 lanes), and the step end over all signals, which clears the group's histograms and
     *  its members' normalisations only: the table is whole after every step, with or without lut_output.
     *  columns_in_place: fill and event sum in one entry instead, the histogram columns looked up in place
     *  (sxmc_group_eval_columns_nll_async; see the flag for what was measured).  consume = false: the plain
     *  step end, the group zeroes itself.  No group: kernel evaluations, nll_event_chunks, step end.  Where nothing is
     *  re-evaluated (no floating systematic) the table of the set-up is summed.  The chain is REFERENCE's bit for bit. */
    void mixed_step() {
      const sxmc_step_args& a = d.a;
      bool summed = false;
      if (form.reevaluate) {
        for (const KernelMember& k : m.kernels)
          if (k.floats) check(sxmc_kde_eval_on_stream_async(k.eval->Handle(), 1, strm));
        if (m.group && m.columns_in_place && !m.lut_output) {
          check(sxmc_group_eval_columns_nll_async(m.group, strm, d.lut, nevents, a.d_v_proposed, a.d_nexpected, a.d_n_mc,
                                                  a.d_source_id, a.d_norms, d.sums, (int)m.nnllblocks,
                                                  (int)m.nllblocksize));
          summed = true;
        } else if (m.group) {
          check(sxmc_group_eval_async(m.group, 1, strm));
        }
      }
      if (!summed) {
        m.event_chunks(strm, d.lut, nevents, a.d_v_proposed, a.d_nexpected, a.d_n_mc, a.d_source_id, a.d_norms, d.sums,
                       d_weights);
      }
      if (m.group && form.reevaluate && m.consume) {
        check(sxmc_group_finish_columns_step_async(m.group, strm, (size_t)m.nnllthreads, d.sums, a.d_means, a.d_sigmas,
                                                   a.d_rng, a.d_nll_current, a.d_nll_proposed, a.d_v_current,
                                                   a.d_v_proposed, a.d_accepted, a.d_counter, a.d_jump_buffer,
                                                   a.nparameters, a.nsources, a.d_jump_width, a.d_nexpected, a.d_n_mc,
                                                   a.d_source_id, a.d_norms, a.debug_mode));
        return;
      }
      SXMC_KERNEL_LAUNCH(finish_nll_jump_pick_combo, 1, m.nreducethreads, m.nreducethreads * sizeof(double), strm,
                         (size_t)m.nnllthreads, d.sums, m.nsignals, m.nsources, a.d_means, a.d_sigmas, a.d_rng,
                         a.d_nll_current, a.d_nll_proposed, a.d_v_current, a.d_v_proposed, a.d_accepted, a.d_counter,
                         a.d_jump_buffer, a.nparameters, a.d_jump_width, a.d_nexpected, a.d_n_mc, a.d_source_id,
                         a.d_norms, debug_mode, d_factor, d_whitening);
    }

    /** The run of steps that starts at step i: what the host does before it (re-tuning, the form of the fill), the
     *  steps in the walk's form, the flush after them.  Returns the first step of the next run. */
    unsigned run(unsigned i) {
      if (plan.retune_due(i)) retune();
      // steps i..f need the host only before the first and after the last
      const unsigned f = plan.run_end(i, two_forms);
      resolve();
      // a plan with a boxed and an ordered form of the fill: the form of the steps up to the next flush, from the
      // parameters the device holds now (sxmc_group_adapt_fill_form); recorded steps replay the old form, so they are
      // recorded again by the run
      if (form.adapts_fill_form()) {
        int fill_form = 0, changed = 0;
        check(sxmc_group_adapt_fill_form(m.group, &fill_form, &changed));
        two_forms = fill_form != 0 && plan.adapt_interval < plan.sync_interval;
        if (changed) check(graph.reset());
      }
      const unsigned n = f - i + 1;
      switch (form.step) {
        case WalkForm::LOCKSTEP: lockstep_run(i, n); break;
        case WalkForm::LOOKAHEAD: lookahead_run(i, n); break;
        default: sequential_run(i, n);
      }
      flush(f);
      return f + 1;
    }

    /** Re-tune the proposal from the burn-in samples (mcmc.cpp:274-311); the width becomes scale_factor x the standard
     *  deviation of the parameter over the steps kept so far */
    void retune() {
      for (size_t j = 0; j < m.nparameters; j++) {
        if (m.parameter_fixed[j]) continue;
        const double sd = column_stddev(chain, j);
        const double fit_width = sd > 0 ? sd : jump_width.readOnlyHostPtr()[j];
        jump_width.hostPtr()[j] = scale_factor * fit_width;
      }
      if (covariance) rebuild_factor(chain.rows.data(), chain.nrows());
      if (!debug_mode) chain.rows.clear();
    }

    /** The factor of the correlated proposal from the rows kept so far and the widths as they now stand: the library's
     *  one implementation (sxmc_proposal_factor), into the walk's one array. */
    void rebuild_factor(const float* rows, size_t nrows) {
      check(sxmc_proposal_factor(rows, nrows, (int)m.nparameters, jump_width.readOnlyHostPtr(), m.proposal_shrinkage,
                                 factor->hostPtr(), &m.last_shrinkage));
      m.last_factor.assign(factor->readOnlyHostPtr(), factor->readOnlyHostPtr() + m.nparameters * m.nparameters);
    }

    /** Set-up is over: the lock goes BEFORE a run is queued -- a run is up to sync_interval steps, a second of device
     *  work at config 3, and whoever holds the lock while that is queued keeps every other chain's set-up waiting.
     *  announce: tell the caller, once (an ensemble's lanes meet there: see MCMC::on_setup_done). */
    void release_before_queueing(bool announce) {
      if (excl.owns_lock()) excl.unlock();
      if (announce && !setup_announced) {
        setup_announced = true;
        if (m.on_setup_done) m.on_setup_done();
      }
    }

    /** n steps launched by this chain: graph replays (split_run) and the remainder one by one.  Lock: the first run
     *  (step 0, eager: it builds the launch plans) keeps it; the first run after it records its graph under the lock,
     *  as it was taken at set-up, and releases it before anything is queued; later runs hold no lock, and re-record
     *  (a changed fill form) without it. */
    void sequential_run(unsigned i, unsigned n) {
      const RunSplit split = split_run(n, form.gsteps, i == 0);
      if (split.replays > 0 && !graph) {
        check(record_graph(strm, m.exclusive, excl.owns_lock(), form.gsteps, graph, [&]() {
          one_step();
          return SXMC_OK;
        }));
      }
      if (i > 0) release_before_queueing(true);
      if (split.replays > 0) check(sxmc_graph_launch(graph.get(), strm, (int)split.replays));
      for (unsigned k = 0; k < split.remainder; k++) one_step();
    }

    /** n steps together with the other chains of the set (recorded and replayed there).  Lock: released before the
     *  chain waits for its partners, who need it for their own set-up; the set takes it itself where it must. */
    void lockstep_run(unsigned i, unsigned n) {
      release_before_queueing(i > 0);
      m.lockstep->advance(m.lockstep_index, m.group, d.a, n, m.graph_steps);
    }

    /** Exactly n steps, taken one or two per pass: passes in rounds of about what is still needed (lookahead_round),
     *  the step counter read back after each round; a pass beyond the stop does nothing (the counter was 0 at the
     *  flush).  Never calls on_setup_done.  Lock: see lookahead_lock. */
    void lookahead_run(unsigned i, unsigned n) {
      Shadow& s = *shadow;
      s.stop.writeOnlyHostPtr()[0] = (int)n;
      const int* d_stop = s.stop.readOnlyPtr();
      double* d_ahead = s.vector.ptr();
      const unsigned* d_anorms = s.norms.ptr();
      // the look-ahead vector for the chain as it stands (new widths after a re-tuning included)
      check(sxmc_lookahead_begin(strm, d.a.nparameters, d.a.d_rng, d.a.d_jump_width, d.a.d_v_current, d_ahead));
      auto one_pass = [&]() {
        check(sxmc_multigroup_lookahead_step_async(s.pair.get(), strm, &d.a, d_ahead, d_anorms, d_stop));
        m.ahead_passes++;
      };
      unsigned done = 0;
      while (done < n) {
        const LookaheadRound round =
            lookahead_round(n - done, m.ahead_steps_seen, m.ahead_passes_seen, form.gsteps, (bool)graph);
        const size_t p0 = m.ahead_passes;
        lookahead_lock(i, round.records);
        if (round.records) {
          one_pass();   // (plans in place before recording)
          s.planned = true;
          check(record_graph(strm, m.exclusive, excl.owns_lock(), form.gsteps, graph, [&]() {
            one_pass();
            return SXMC_OK;
          }));
          m.ahead_passes -= form.gsteps;   // (recorded, not launched)
          if (i > 0 && excl.owns_lock()) excl.unlock();   // released after the recording
        }
        if (round.replays > 0) {
          check(sxmc_graph_launch(graph.get(), strm, (int)round.replays));
          m.ahead_passes += (size_t)round.replays * form.gsteps;
        }
        for (unsigned q = 0; q < round.single_passes; q++) {
          one_pass();
          if (!s.planned) {
            s.planned = true;
            if (i > 0 && excl.owns_lock()) excl.unlock();   // released after the pair's first pass
          }
        }
        (void)jump_counter.ptr();   // (the device side changed behind the mirror's back: the host copy is stale)
        const unsigned now = (unsigned)jump_counter.readOnlyHostPtr()[0];   // (a blocking copy on the chain's stream)
        if (now <= done && now < n) throw pdfz::Error("look-ahead walk: the chain did not advance");
        m.ahead_steps_seen += now - done;
        m.ahead_passes_seen += m.ahead_passes - p0;
        done = now;
      }
    }

    /** The pair's first pass builds its launch plans (allocations, a module load, a device-wide synchronisation) and a
     *  recording must not meet another thread's allocation: a round that does either takes the set-up lock, like the
     *  sequential walk's recording.  Every other round only launches and waits on this chain's stream: after the first
     *  run it holds no lock.  (The first run keeps the lock, as the sequential walk's does.) */
    void lookahead_lock(unsigned i, bool records) {
      if (!m.exclusive) return;
      if (!shadow->planned || records) {
        if (!excl.owns_lock()) excl.lock();
      } else if (i > 0 && excl.owns_lock()) {
        excl.unlock();
      }
    }

    /** Flush the jump buffer after step f (mcmc.cpp:351-377); the host reads go through blocking copies.  Lock: as the
     *  run left it. */
    void flush(unsigned f) {
      const int njumps = jump_counter.readOnlyHostPtr()[0];
      const int naccepted = accept_counter.readOnlyHostPtr()[0];
      if (m.verbose) {
        std::printf("MCMC: Step %u/%u (%d in buffer, %d accepted)\n", f + 1, plan.nsteps, njumps, naccepted);
      }
      const float* jb = jump_buffer.readOnlyHostPtr();
      chain.rows.insert(chain.rows.end(), jb, jb + (size_t)njumps * ncol);
      chain.accepted += (size_t)naccepted;
      jump_counter.writeOnlyHostPtr()[0] = 0;
      accept_counter.writeOnlyHostPtr()[0] = 0;
      if (form.batched) {
        // the cooperative step end waits inside its kernel, with a bound: a wait that ran into it left the steps of
        // this run invalid -- never seen on a healthy device, and not to be passed on silently if it ever happens
        unsigned timeouts = 0;
        check(sxmc_group_step_end_timeouts(m.group, strm, &timeouts));
        if (timeouts) {
          throw pdfz::Error("MCMC: " + std::to_string(timeouts) + " workgroup(s) of the cooperative step end gave up "
                            "waiting (sxmc_group_step_end_timeouts): the chain is not valid");
        }
      }
    }

    /** The end of a walk that went well: the caller's hook once the last step has finished, the tear-down with its
     *  errors thrown, the final wait. */
    Chain finish(std::chrono::steady_clock::time_point steps_t0) {
      if (strm) check(sxmc_stream_synchronize(strm));
      chain.steps_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - steps_t0).count();
      if (m.on_steps_done) m.on_steps_done();
      tear_down(false);
      if (m.stream) {
        check(sxmc_stream_synchronize(m.stream));  // this chain only: others may be running beside it
      } else {
        check(sxmc_device_synchronize());
      }
      return std::move(chain);
    }

    /** What every walk leaves behind, however it ended.  unwinding: the walk failed -- wait for what it queued first
     *  (finish() has waited already), and report nothing: the walk's own exception is the one that travels on. */
    void tear_down(bool unwinding) {
      torn_down = true;
      if (unwinding) (void)(strm ? sxmc_stream_synchronize(strm) : sxmc_device_synchronize());
      int rc_graph = SXMC_OK, rc_stream = SXMC_OK;
      auto release = [&]() {   // tear-down frees device memory: under the lock, and the arrays die under it too
        if (m.exclusive && !excl.owns_lock()) excl.lock();
        rc_graph = graph.reset();
        rc_stream = own_stream.reset();
      };
      try {
        // the evaluators borrowed this walk's arrays (lookup table, normalisations, parameter vectors): un-bind them
        // before the arrays die, or the next evaluation of an evaluator would touch destroyed arrays
        // (a mixed walk launched its kernel members on this walk's stream, which they remember: they let go of it
        //  here, while it exists -- everything on it has been waited for)
        if (form.step == WalkForm::MIXED)
          for (const KernelMember& k : m.kernels) k.eval->EvalFinished();
        for (pdfz::Eval* p : m.pdfs) p->ForgetBuffers();
        if (m.group) (void)sxmc_group_set_proposal_factor(m.group, nullptr);   // (it borrowed this walk's factor)
        if (m.group) (void)sxmc_group_set_constraint_whitening(m.group, nullptr);   // (and its whitening matrix)
        if (shadow)
          for (auto& p : shadow->evaluators) p->ForgetBuffers();
        // (before the lock is re-taken: the set's launcher takes the two in the other order)
        if (m.lockstep) m.lockstep->leave(m.lockstep_index);
      } catch (...) {
        release();   // whatever those threw, nothing is freed outside the lock
        throw;
      }
      release();
      if (!unwinding) {
        check(rc_graph);
        check(rc_stream);
      }
    }
  };
  sxmc_stream_t stream;  //!< every launch of this chain goes here (null: the legacy default stream, as the
                         //!< reference; one non-blocking stream per chain when several run on one GPU)
  size_t nsources, nsignals, nsystematics, nobservables;
  size_t nparameters = 0, nfloat = 0;
  bool systematics_fixed = true;
  unsigned nnllblocks, nllblocksize, nnllthreads, nreducethreads;
  std::unique_ptr<pdfz::Array<double>> parameter_means, parameter_sigma, nexpected;
  std::unique_ptr<pdfz::Array<unsigned>> n_mc;
  std::unique_ptr<pdfz::Array<short>> source_id;
  std::unique_ptr<pdfz::Array<RNGState>> rngs;
  std::vector<std::string> parameter_names;
  std::vector<bool> parameter_fixed;
  std::vector<pdfz::Eval*> pdfs;
  sxmc_group_t group = nullptr;
  /** A kernel-density member of a mixed fit.  floats: one of the parameters its systematics read is not fixed (asked of
   *  the evaluator at every walk); the others keep the column and the norm of the set-up evaluation -- the evaluation is
   *  deterministic, so skipping it leaves the chain unchanged. */
  struct KernelMember {
    pdfz::EvalKernel* eval;
    bool floats;
  };
  std::vector<KernelMember> kernels;   //!< non-empty: every evaluator is an EvalHist or an EvalKernel (the walk is MIXED)
  const char* form_name = "reference";
  std::vector<double> last_factor;     //!< ProposalFactor(): the last COVARIANCE walk's factor, as the device read it
  double last_shrinkage = 0;
  std::vector<double> last_whitening;  //!< ConstraintWhitening(): the last constrained walk's matrix, as the device read it
  bool optimized = false;
  size_t ahead_passes = 0, ahead_passes_seen = 0;   //!< look-ahead walk: passes launched / counted in the rate below
  double ahead_steps_seen = 0;
};

}  // namespace sxmc
