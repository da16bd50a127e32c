// experiment.h -- the experiment loop of the reference (src/sxmc.cpp:59-145) on one GPU: one experiment (fake data ->
// MCMC -> intervals -> report), and the runners that put many of them on a device -- one after the other (ensemble),
// in concurrent lanes (ensemble_concurrent), in lockstep sets (ensemble_lockstep).  Every runner gives the results of
// `ensemble`: an experiment is seeded by its index.  The runners' settings are ONE struct (ExperimentOptions); a lane
// -- host thread, stream, evaluators that share the resident tables, copies of the fit's description -- is set up and
// torn down in ONE place (run_lane).
#pragma once

#include <chrono>
#include <cstdio>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "fake_data.h"
#include "intervals.h"
#include "lane_sync.h"
#include "mcmc.h"

namespace sxmc {

/** sxmc.cpp:130-141 writes every experiment's sampled likelihood space ("ls") to <output_prefix>_<i>.root.  Set this to
 *  receive the chains (experiment index, chain) -- e.g. to write them with write_chain_npz (config.h).  Called on the
 *  experiment's own host thread; calls are serialised.  Empty by default: chains are dropped once their intervals are
 *  taken. */
inline std::function<void(unsigned, const Chain&)>& chain_sink() {
  static std::function<void(unsigned, const Chain&)> sink;
  return sink;
}

/** Set by a caller whose configuration lists data sets (sxmc.cpp:71-80): asked for experiment k's events (rows of
 *  nobservables + 1 floats); true = `rows` holds them, false = the experiment samples a fake data set as usual.  May be
 *  called from several host threads at once (one per chain in flight): it must only read. */
inline std::function<bool(unsigned, std::vector<float>&)>& data_source() {
  static std::function<bool(unsigned, std::vector<float>&)> source;
  return source;
}

/** Set by a caller that wants what sxmc.cpp:100-101 prints for every experiment -- the text of print_best_fit followed
 *  by print_correlations -- handed over as (experiment index, text), one call at a time. */
inline std::function<void(unsigned, const std::string&)>& report_sink() {
  static std::function<void(unsigned, const std::string&)> sink;
  return sink;
}

/** A chain from a table of columns (parameter names..., "likelihood"): what read_table (config.h) returns for a file
 *  written by write_chain_npz / sxmc_amd/io.py -- the `fit.samples` path of sxmc.cpp:84-94, where a saved likelihood
 *  space replaces the walk. */
inline Chain chain_from_table(const std::vector<float>& matrix, const std::vector<std::string>& fields) {
  if (fields.empty() || fields.back() != "likelihood" || matrix.size() % fields.size() != 0 || matrix.empty()) {
    throw pdfz::Error("a saved chain needs at least one row and \"likelihood\" as its last column");
  }
  Chain c;
  c.names = fields;
  c.rows = matrix;
  return c;
}

struct ExperimentResult {
  unsigned index = 0;
  std::vector<Interval> intervals;  //!< one per parameter
  size_t accepted = 0;
  size_t nevents = 0;
  /** where the experiment's host time went (seconds): its data (fake-data draw or configured files), the chain's
   *  construction, the walk's set-up (buffers, SetEvalPoints, first evaluation), its steps, its tear-down (buffers
   *  freed), the chain's destruction, the intervals.  What a short experiment spends outside `steps` is what an
   *  ensemble of short experiments loses (bench_cpp prints the sums). */
  struct Phases {
    double data = 0, construct = 0, walk_setup = 0, steps = 0, walk_teardown = 0, destroy = 0, intervals = 0;
  } phases;
};

/** Per-experiment seed (the reference's single sequential gRandom stream cannot be sharded). */
inline unsigned long long experiment_seed(unsigned long long base_seed, unsigned k) {
  unsigned long long x = base_seed * 0x9E3779B97F4A7C15ull + (k + 1ull) * 0xBF58476D1CE4E5B9ull;
  x ^= x >> 31;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 29;
  return x;
}

/** What the runners below can be told.  The positional overloads spell the first four (and device, device_exclusive)
 *  out as arguments and forward here. */
struct ExperimentOptions {
  float cl = 0.9f;
  unsigned sync_interval = 10000;
  unsigned graph_steps = 0;
  ErrorType error_type = ERROR_CONTOUR;   //!< fit.error_type: contour or projection intervals
  bool optimize = true;   //!< MCMC::optimize of every chain the runner builds (chains of a lockstep set: always false)
  int device = -1;        //!< >= 0: the lanes' host threads select this device
  /** set-up, graph recording and tear-down of the lanes take this lock instead of one of the call's own
   *  (ensemble_multi_gpu passes the device's, so that lanes of one card started from different calls still take turns) */
  SetupLock* device_exclusive = nullptr;
  Proposal proposal = Proposal::DIAGONAL;   //!< MCMC::proposal of every chain the runner builds (fit.proposal);
  double proposal_shrinkage = 0.05;         //!< ensemble_lockstep refuses COVARIANCE: its sets have no such step end
  std::vector<double> constraint_correlation = {};   //!< MCMC::constraint_correlation of every chain the runner builds (the
                                            //!< fit's constraint_correlations, scattered); ensemble_lockstep refuses it
  bool asimov = false;   //!< fit.asimov: fit exactly ONE data set, the Asimov one (make_asimov_dataset: weighted events) --
                         //!< ensemble and ensemble_concurrent then run the first of `experiments` alone and say so through
                         //!< the report; ensemble_lockstep and ensemble_multi_gpu refuse it (no weighted lockstep step
                         //!< end; one fit needs one card)
};

/** Where an experiment runs when it is one of several in flight: all "none" for the one-at-a-time loop. */
struct LaneContext {
  sxmc_stream_t stream = nullptr;     //!< null: the default stream
  SetupLock* exclusive = nullptr;     //!< one chain per host thread: held over everything that allocates, copies through
                                      //!< the legacy stream or synchronises the device -- see MCMC::exclusive
  LockstepSet* lockstep = nullptr;    //!< the chain steps with the other chains of this set, as its lockstep_index-th
  size_t lockstep_index = 0;
  LaneBarrier* meet = nullptr;        //!< the lanes of a round meet here (see LaneBarrier), meet_lanes of them
  size_t meet_lanes = 0;
};

namespace detail {

typedef std::chrono::steady_clock PhaseClock;
inline double since(PhaseClock::time_point t) { return std::chrono::duration<double>(PhaseClock::now() - t).count(); }

/** The lanes of one round meet when all are set up and when all have stepped; a walk that ends without having passed a
 *  meeting point -- a form that has none -- passes it afterwards, so that nobody waits for it; one that throws breaks
 *  the barrier. */
struct Meeting {
  LaneBarrier* meet;
  size_t lanes;
  bool met_setup = false, met_steps = false;
  bool several() const { return meet && lanes > 1; }
  void attach(MCMC& mcmc) {
    if (!several()) return;
    mcmc.on_setup_done = [this]() {
      met_setup = true;
      meet->arrive_and_wait(lanes);
    };
    mcmc.on_steps_done = [this]() {
      met_steps = true;
      meet->arrive_and_wait(lanes);
    };
  }
  Chain walk(MCMC& mcmc, std::vector<float>& data, unsigned nsteps, float burnin_fraction, unsigned sync_interval,
             const std::vector<double>* event_weights = nullptr) {
    Chain chain;
    try {
      chain = event_weights ? mcmc(data, *event_weights, nsteps, burnin_fraction, false, sync_interval)
                            : mcmc(data, nsteps, burnin_fraction, false, sync_interval);
    } catch (...) {
      if (meet) meet->break_all();
      throw;
    }
    if (several()) {
      if (!met_setup) meet->arrive_and_wait(lanes);
      if (!met_steps) meet->arrive_and_wait(lanes);
    }
    return chain;
  }
};

/** Experiment k's events: the configured data set when there is one, a fake data set otherwise. */
inline std::vector<float> experiment_data(unsigned k, std::mt19937_64& rng, std::vector<Signal>& signals,
                                          std::vector<Systematic>& systematics, std::vector<Observable>& observables) {
  std::vector<float> data;
  if (!(data_source() && data_source()(k, data))) data = make_fake_dataset(rng, signals, systematics, observables, true);
  return data;
}

inline std::unique_ptr<MCMC> experiment_chain(std::vector<Source>& sources, std::vector<Signal>& signals,
                                              std::vector<Systematic>& systematics, std::vector<Observable>& observables,
                                              unsigned long long seed, const ExperimentOptions& opt,
                                              const LaneContext& lane) {
  std::unique_ptr<MCMC> mcmc(new MCMC(sources, signals, systematics, observables, seed, lane.stream));
  mcmc->graph_steps = opt.graph_steps;
  mcmc->proposal = opt.proposal;
  mcmc->proposal_shrinkage = opt.proposal_shrinkage;
  mcmc->constraint_correlation = opt.constraint_correlation;
  mcmc->exclusive = lane.exclusive;
  mcmc->lockstep = lane.lockstep;
  mcmc->lockstep_index = lane.lockstep_index;
  // chains that share a fill pass share ONE launch shape: the default one
  mcmc->optimize = opt.optimize && !lane.lockstep;
  return mcmc;
}

/** The chain to its sink, its intervals, and what sxmc.cpp:100-101 prints to the report's. */
inline void experiment_report(unsigned k, const Chain& chain, const ExperimentOptions& opt, ExperimentResult& r) {
  if (chain_sink()) {
    static std::mutex sink_mutex;
    std::lock_guard<std::mutex> guard(sink_mutex);
    chain_sink()(k, chain);
  }
  const PhaseClock::time_point t = PhaseClock::now();
  r.intervals = extract_intervals(chain, opt.cl, opt.error_type);
  r.phases.intervals = since(t);
  r.accepted = chain.accepted;
  if (report_sink()) {
    std::ostringstream os;
    print_best_fit(os, chain, r.intervals);
    print_correlations(os, chain);
    static std::mutex report_mutex;
    std::lock_guard<std::mutex> guard(report_mutex);
    report_sink()(k, os.str());
  }
}

}  // namespace detail

/** One iteration of sxmc.cpp:59-145: data -> MCMC -> intervals.  With lane.exclusive the lock is held over the data
 *  and the chain's construction, by the walk where it needs it, and over the chain's destruction. */
inline ExperimentResult run_experiment(unsigned k, unsigned long long base_seed, std::vector<Source>& sources,
                                       std::vector<Signal>& signals, std::vector<Systematic>& systematics,
                                       std::vector<Observable>& observables, unsigned nsteps, float burnin_fraction,
                                       const ExperimentOptions& opt, const LaneContext& lane = LaneContext()) {
  using detail::PhaseClock;
  using detail::since;
  const unsigned long long x = experiment_seed(base_seed, k);
  std::mt19937_64 rng(x);
  std::unique_lock<SetupLock> lock;
  if (lane.exclusive) lock = std::unique_lock<SetupLock>(*lane.exclusive);
  ExperimentResult r;
  r.index = k;
  PhaseClock::time_point t = PhaseClock::now();
  std::vector<float> data;
  std::vector<double> weights;
  if (opt.asimov) {
    if (lane.lockstep) {
      throw pdfz::Error("run_experiment: a lockstep set has no weighted step end: fit the Asimov data set in a chain of its own");
    }
    AsimovDataset a = make_asimov_dataset(signals, systematics, observables);
    data = std::move(a.events);
    weights = std::move(a.weights);
    if (report_sink()) {
      double total = 0;
      for (double w : weights) total += w;
      char line[160];
      std::snprintf(line, sizeof line, "Fitting the Asimov data set: %zu weighted rows, %.17g expected events\n",
                    weights.size(), total);
      report_sink()(k, line);
    }
  } else {
    data = detail::experiment_data(k, rng, signals, systematics, observables);
  }
  r.nevents = data.size() / (observables.size() + 1);
  r.phases.data = since(t);
  t = PhaseClock::now();
  std::unique_ptr<MCMC> mcmc = detail::experiment_chain(sources, signals, systematics, observables, x, opt, lane);
  detail::Meeting meeting{lane.meet, lane.meet_lanes};
  meeting.attach(*mcmc);
  r.phases.construct = since(t);
  if (lane.exclusive) lock.unlock();   // the walk takes it itself
  t = PhaseClock::now();
  const Chain chain = meeting.walk(*mcmc, data, nsteps, burnin_fraction, opt.sync_interval, opt.asimov ? &weights : nullptr);
  r.phases.walk_setup = chain.setup_seconds;
  r.phases.steps = chain.steps_seconds;
  r.phases.walk_teardown = since(t) - chain.setup_seconds - chain.steps_seconds;
  t = PhaseClock::now();
  if (lane.exclusive) lock.lock();
  mcmc.reset();
  if (lane.exclusive) lock.unlock();
  r.phases.destroy = since(t);
  detail::experiment_report(k, chain, opt, r);
  return r;
}

/** The experiment loop of sxmc.cpp:59-145 over the given experiment indices (all of them on one GPU, or this rank's
 *  share), one at a time.  Evaluators (and their MC tables in HBM) are reused by every experiment. */
inline std::vector<ExperimentResult> ensemble(const std::vector<unsigned>& experiments, unsigned long long base_seed,
                                              std::vector<Source>& sources, std::vector<Signal>& signals,
                                              std::vector<Systematic>& systematics,
                                              std::vector<Observable>& observables, unsigned nsteps,
                                              float burnin_fraction, const ExperimentOptions& opt) {
  PoolScope pool;   // the experiments' arrays recycle their blocks instead of allocating and freeing (device_array.h)
  std::vector<ExperimentResult> out;
  for (unsigned k : experiments) {
    out.push_back(run_experiment(k, base_seed, sources, signals, systematics, observables, nsteps, burnin_fraction, opt));
    if (opt.asimov) break;   // (exactly one data set, the expected one: every further experiment would fit it again)
  }
  return out;
}

inline std::vector<ExperimentResult> ensemble(const std::vector<unsigned>& experiments, unsigned long long base_seed,
                                              std::vector<Source>& sources, std::vector<Signal>& signals,
                                              std::vector<Systematic>& systematics,
                                              std::vector<Observable>& observables, unsigned nsteps,
                                              float burnin_fraction, float cl = 0.9f, unsigned sync_interval = 10000,
                                              unsigned graph_steps = 0, ErrorType error_type = ERROR_CONTOUR) {
  return ensemble(experiments, base_seed, sources, signals, systematics, observables, nsteps, burnin_fraction,
                  ExperimentOptions{cl, sync_interval, graph_steps, error_type, true, -1, nullptr});
}

namespace detail {

/** What a lane's body works with: its stream, and its own evaluators and copies of the fit's description. */
struct Lane {
  sxmc_stream_t stream = nullptr;
  std::vector<Source> sources;
  std::vector<Signal> signals;   //!< evaluators of this lane that share the resident sample tables (share_pdfz)
  std::vector<Systematic> systematics;
  std::vector<Observable> observables;
};

/** One lane of experiments in flight, on the calling host thread.  Set-up: the device is selected (a per-thread
 *  setting); under the lock the lane takes `adopted` as its stream or, when that is null, creates a non-blocking one
 *  of its own, makes it the thread's transfer stream and gets its evaluators; outside the lock it copies sources,
 *  systematics and observables.  Then body(lane).  Whatever is thrown is kept in `error`, and failed(message) tells
 *  the lane's peers.  Tear-down, under the lock: the evaluators, the transfer stream, the stream if the lane created it. */
template <typename Body, typename Failed>
void run_lane(const ExperimentOptions& opt, SetupLock& exclusive, sxmc_stream_t adopted,
              const std::vector<Source>& sources, const std::vector<Signal>& signals,
              const std::vector<Systematic>& systematics, const std::vector<Observable>& observables,
              std::exception_ptr& error, Body&& body, Failed&& failed) {
  Lane lane;
  OwnedStream own;
  try {
    if (opt.device >= 0) check(sxmc_set_device(opt.device));   // (the current device is a per-thread setting)
    {
      std::lock_guard<SetupLock> lock(exclusive);
      if (!adopted) check(sxmc_stream_create_nonblocking(own.put()));
      lane.stream = adopted ? adopted : own.get();
      transfer_stream() = lane.stream;
      for (const Signal& s : signals) lane.signals.push_back(share_pdfz(s));
    }
    lane.sources = sources;
    lane.systematics = systematics;
    lane.observables = observables;
    body(lane);
  } catch (const pdfz::Error& e) {
    error = std::current_exception();
    failed(e.msg);
  } catch (const std::exception& e) {
    error = std::current_exception();
    failed(e.what());
  } catch (...) {
    error = std::current_exception();
    failed("a chain of the set failed");
  }
  std::lock_guard<SetupLock> lock(exclusive);
  for (Signal& s : lane.signals) delete s.histogram;
  transfer_stream() = nullptr;
  own.reset();
}

/** lane(t, error of lane t) on a host thread per lane; when all have ended, the lowest-numbered lane's exception. */
template <typename LaneFn>
void run_lanes(size_t lanes, LaneFn&& lane) {
  std::vector<std::exception_ptr> errors(lanes);
  std::vector<std::thread> threads;
  for (size_t t = 0; t < lanes; t++) threads.emplace_back([&, t]() { lane(t, errors[t]); });
  for (std::thread& th : threads) th.join();
  for (std::exception_ptr& e : errors)
    if (e) std::rethrow_exception(e);
}

}  // namespace detail

/** The same loop with `nconcurrent` experiments in flight on this GPU (BASELINE config 4's per-GPU shape:
 *  one experiment per stream).  Each lane is a host thread with its own non-blocking stream and its own
 *  evaluators, which share the resident sample tables of `signals` (share_pdfz); lane t runs experiments
 *  t, t + nconcurrent, ...  Results come back in the order of `experiments` and are the ones `ensemble`
 *  gives (every experiment is seeded by its index). */
inline std::vector<ExperimentResult> ensemble_concurrent(const std::vector<unsigned>& experiments,
                                                         unsigned long long base_seed, std::vector<Source>& sources,
                                                         std::vector<Signal>& signals,
                                                         std::vector<Systematic>& systematics,
                                                         std::vector<Observable>& observables, unsigned nsteps,
                                                         float burnin_fraction, unsigned nconcurrent,
                                                         const ExperimentOptions& opt) {
  if (opt.asimov) {   // (one fit: nothing to run beside it)
    return ensemble(experiments, base_seed, sources, signals, systematics, observables, nsteps, burnin_fraction, opt);
  }
  PoolScope pool;   // the experiments' arrays recycle their blocks instead of allocating and freeing (device_array.h)
  const size_t lanes = std::max<size_t>(1, std::min<size_t>(nconcurrent, experiments.size()));
  std::vector<ExperimentResult> out(experiments.size());
  SetupLock own_exclusive;
  SetupLock& exclusive = opt.device_exclusive ? *opt.device_exclusive : own_exclusive;
  LaneBarrier meet;    // the lanes walk in ROUNDS: set up one after the other, step side by side, tear down
  detail::run_lanes(lanes, [&](size_t t, std::exception_ptr& error) {
    detail::run_lane(
        opt, exclusive, nullptr, sources, signals, systematics, observables, error,
        [&](detail::Lane& lane) {
          for (size_t i = t; i < experiments.size(); i += lanes) {
            LaneContext where;
            where.stream = lane.stream;
            where.exclusive = &exclusive;
            where.meet = &meet;
            // (lanes in this round: all of them, or what is left of the list in its last round)
            where.meet_lanes = std::min(lanes, experiments.size() - (i - t));
            out[i] = run_experiment(experiments[i], base_seed, lane.sources, lane.signals, lane.systematics,
                                    lane.observables, nsteps, burnin_fraction, opt, where);
          }
        },
        [&](const std::string&) { meet.break_all(); });
  });
  return out;
}

inline std::vector<ExperimentResult> ensemble_concurrent(const std::vector<unsigned>& experiments,
                                                         unsigned long long base_seed, std::vector<Source>& sources,
                                                         std::vector<Signal>& signals,
                                                         std::vector<Systematic>& systematics,
                                                         std::vector<Observable>& observables, unsigned nsteps,
                                                         float burnin_fraction, unsigned nconcurrent, float cl = 0.9f,
                                                         unsigned sync_interval = 10000, unsigned graph_steps = 0,
                                                         int device = -1, SetupLock* device_exclusive = nullptr,
                                                         ErrorType error_type = ERROR_CONTOUR) {
  return ensemble_concurrent(experiments, base_seed, sources, signals, systematics, observables, nsteps,
                             burnin_fraction, nconcurrent,
                             ExperimentOptions{cl, sync_interval, graph_steps, error_type, true, device, device_exclusive});
}

/** The same loop with the experiments in flight advanced in LOCKSTEP sets (BASELINE config 4's per-GPU shape, taken
 *  further): `nsets` sets of `chains_per_set` chains; the chains of a set walk on one stream and share ONE pass
 *  over the sample tables per step (LockstepSet / sxmc_multigroup_step_async: the bytes streamed per evaluation
 *  divide by the chains per set; config 3: 9 500 steps/s with 2 sets of 4 against 5 500 with a fill per chain),
 *  different sets run on different streams so that one set's step ends overlap another's fill.  Every lane is a
 *  host thread, as in ensemble_concurrent; experiments that do not fill a whole round of nsets x chains_per_set
 *  lanes run through ensemble_concurrent at the end.  Results are those of `ensemble`, in the order of
 *  `experiments`. */
inline std::vector<ExperimentResult> ensemble_lockstep(const std::vector<unsigned>& experiments,
                                                       unsigned long long base_seed, std::vector<Source>& sources,
                                                       std::vector<Signal>& signals, std::vector<Systematic>& systematics,
                                                       std::vector<Observable>& observables, unsigned nsteps,
                                                       float burnin_fraction, unsigned chains_per_set, unsigned nsets,
                                                       const ExperimentOptions& opt) {
  if (!opt.constraint_correlation.empty()) {
    throw pdfz::Error("ensemble_lockstep: a lockstep set has no step end with correlated constraints: run an ensemble "
                      "with a constraint_correlation one experiment per chain (ensemble, ensemble_concurrent)");
  }
  if (opt.proposal == Proposal::COVARIANCE) {
    throw pdfz::Error("ensemble_lockstep: a lockstep set has no correlated step end: run a COVARIANCE ensemble one "
                      "experiment per chain (ensemble, ensemble_concurrent)");
  }
  if (opt.asimov) {
    throw pdfz::Error("ensemble_lockstep: a lockstep set has no weighted step end: fit the Asimov data set with ensemble");
  }
  for (const Signal& s : signals) {
    if (!s.multiplicities.empty()) {
      throw pdfz::Error("ensemble_lockstep: signal '" + s.name + "' has sample multiplicities and a lockstep set has no "
                        "weighted fill: run the ensemble one experiment per chain (ensemble, ensemble_concurrent)");
    }
  }
  PoolScope pool;  // the experiments' arrays recycle their blocks instead of allocating and freeing (device_array.h)
  const size_t L = std::max(2u, std::min(4u, chains_per_set)), S = std::max(1u, nsets), lanes = L * S;
  const size_t usable = experiments.size() / lanes * lanes;
  std::vector<ExperimentResult> out(experiments.size());
  SetupLock own_exclusive;
  SetupLock& exclusive = opt.device_exclusive ? *opt.device_exclusive : own_exclusive;
  if (usable) {
    // the sets' streams exist before the lanes start, and outlive the sets (declared first: destroyed last)
    std::vector<OwnedStream> streams(S);
    std::vector<std::unique_ptr<LockstepSet>> sets;
    if (opt.device >= 0) check(sxmc_set_device(opt.device));
    for (size_t k = 0; k < S; k++) {
      check(sxmc_stream_create_nonblocking(streams[k].put()));
      sets.emplace_back(new LockstepSet(L, streams[k].get(), &exclusive));
    }
    detail::run_lanes(lanes, [&](size_t t, std::exception_ptr& error) {
      LockstepSet& set = *sets[t / L];
      detail::run_lane(
          opt, exclusive, set.stream, sources, signals, systematics, observables, error,
          [&](detail::Lane& lane) {
            LaneContext where;
            where.stream = set.stream;
            where.exclusive = &exclusive;
            where.lockstep = &set;
            where.lockstep_index = t % L;
            for (size_t i = t; i < usable; i += lanes) {
              out[i] = run_experiment(experiments[i], base_seed, lane.sources, lane.signals, lane.systematics,
                                      lane.observables, nsteps, burnin_fraction, opt, where);
            }
          },
          [&](const std::string& message) { set.abandon(message); });
    });
  }
  if (usable < experiments.size()) {
    std::vector<unsigned> rest(experiments.begin() + (std::ptrdiff_t)usable, experiments.end());
    ExperimentOptions mine = opt;
    mine.device_exclusive = &exclusive;
    std::vector<ExperimentResult> r = ensemble_concurrent(rest, base_seed, sources, signals, systematics, observables,
                                                          nsteps, burnin_fraction, (unsigned)lanes, mine);
    for (size_t i = 0; i < r.size(); i++) out[usable + i] = r[i];
  }
  return out;
}

inline std::vector<ExperimentResult> ensemble_lockstep(const std::vector<unsigned>& experiments,
                                                       unsigned long long base_seed, std::vector<Source>& sources,
                                                       std::vector<Signal>& signals, std::vector<Systematic>& systematics,
                                                       std::vector<Observable>& observables, unsigned nsteps,
                                                       float burnin_fraction, unsigned chains_per_set, unsigned nsets,
                                                       float cl = 0.9f, unsigned sync_interval = 10000,
                                                       unsigned graph_steps = 10, int device = -1,
                                                       SetupLock* device_exclusive = nullptr,
                                                       ErrorType error_type = ERROR_CONTOUR) {
  return ensemble_lockstep(experiments, base_seed, sources, signals, systematics, observables, nsteps, burnin_fraction,
                           chains_per_set, nsets,
                           ExperimentOptions{cl, sync_interval, graph_steps, error_type, true, device, device_exclusive});
}

}  // namespace sxmc
