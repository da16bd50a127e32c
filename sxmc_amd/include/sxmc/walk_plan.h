// walk_plan.h -- the schedule of sxmc::MCMC's walk (mcmc.h) as pure functions: which steps end a run, where the
// proposal widths are re-tuned, how a run splits into graph replays and a remainder, how many look-ahead passes a
// round launches.  No library call and no project header: the standard library only, so that
// tests/cpp/test_walk_plan.cpp checks every rule here without a device.  mcmc.h calls these and keeps no second copy of
// any of them.
#pragma once

#include <algorithm>
#include <cstddef>

namespace sxmc {

/** The steps of a walk that need the host.  A RUN is a stretch of steps i..run_end(i): the host works only before
 *  its first step (re-tuning) and after its last (the jump buffer is read back, mcmc.cpp:351-377).  The arithmetic is
 *  unsigned on purpose: with burnin_steps == 0 the terms burnin_steps - 1 and 2 * burnin_steps - 1 wrap and never
 *  match a step, and step 0 re-tunes; with nsteps == 0 there is no step to ask about.  sync_interval > 0. */
struct WalkSchedule {
  unsigned nsteps, burnin_steps, sync_interval;
  unsigned adapt_interval;   //!< a plan with two forms of the fill: extra flushes every so many steps (0: none)

  /** Is the jump buffer read back after step i?  two_forms: the plan holds a boxed and an ordered form of the fill. */
  bool flush_due(unsigned i, bool two_forms) const {
    return i % sync_interval == 0 || i == nsteps - 1 || i == burnin_steps - 1 || i == 2 * burnin_steps - 1 ||
           (two_forms && adapt_interval > 0 && i % adapt_interval == adapt_interval - 1);
  }
  /** The last step of the run that starts at step i < nsteps (the walk's last step is always due). */
  unsigned run_end(unsigned i, bool two_forms) const {
    unsigned f = i;
    while (!flush_due(f, two_forms)) f++;
    return f;
  }
  /** Are the proposal widths re-tuned before step i (mcmc.cpp:274-311)?  Such a step always starts a run. */
  bool retune_due(unsigned i) const { return i == burnin_steps || i == 2 * burnin_steps; }
};

/** A run of n steps as graph replays of graph_steps recorded steps and a remainder launched one by one. */
struct RunSplit {
  unsigned replays, remainder;
};
/** Replays only after the eager first run (its step builds the launch plans a recording needs), only with
 *  graph_steps > 0 and only when a whole graph fits. */
inline RunSplit split_run(unsigned n, unsigned graph_steps, bool first_run) {
  if (graph_steps == 0 || first_run || n < graph_steps) return RunSplit{0, n};
  return RunSplit{n / graph_steps, n % graph_steps};
}

/** One round of the look-ahead walk: passes launched before the step counter is read back. */
struct LookaheadRound {
  bool records;             //!< one eager pass (it builds the pair's launch plans), then graph_steps passes recorded
                            //!< as a graph, before the replays
  unsigned replays;         //!< replays of the graph (graph_steps passes each)
  unsigned single_passes;   //!< passes launched one by one after them
};
/** need > 0 steps are still to take and a pass takes one or two: about need / rate passes, the rate being 1.75 steps
 *  per pass until 16 passes have been counted and 1.03 x the rate seen afterwards (at most 2); never fewer than one.
 *  More passes than a graph holds go as replays, recorded first when there is no graph yet. */
inline LookaheadRound lookahead_round(unsigned need, double steps_seen, size_t passes_seen, unsigned graph_steps,
                                      bool have_graph) {
  const double rate = passes_seen >= 16 ? std::min(2.0, 1.03 * steps_seen / passes_seen) : 1.75;
  unsigned k = std::max(1u, (unsigned)(need / rate));
  LookaheadRound r{false, 0, 0};
  if (graph_steps > 0 && k > graph_steps) {
    if (!have_graph) {
      r.records = true;
      k--;   // (the eager pass)
    }
    r.replays = k / graph_steps;
    k %= graph_steps;
  }
  r.single_passes = k;
  return r;
}

/** What a walk was asked for and was built over: constant for the whole walk. */
struct WalkFlags {
  bool has_group;          //!< every evaluator is a histogram evaluator of this library: they form a group
  bool reference_form;     //!< the caller wants the reference's own sequence of entry points
  bool systematics_float;  //!< the PDFs are re-evaluated at every step
  bool consume, lut_output;
  bool in_lockstep_set;    //!< the chain was given a lockstep set
  bool lookahead_asked;    //!< lookahead or lookahead_auto
  size_t nparameters;
  unsigned graph_steps;
  bool mixed = false;      //!< there are kernel-density members, and every evaluator is a histogram or kernel-density
                           //!< evaluator of this library; has_group then says whether there are histogram members
  bool covariance_proposal = false;   //!< the proposal is the correlated one: every sequential form takes it, the
                                     //!< look-ahead pass and lockstep sets have no such step end
  bool event_weights = false;         //!< the data events carry real weights: every sequential form takes them (the
                                     //!< reference form and the MIXED form through the weighted launch point, the batched
                                     //!< forms through the group); never LOOKAHEAD or LOCKSTEP
  bool sample_weights = false;        //!< a histogram member carries sample multiplicities (weighted Monte Carlo): every
                                     //!< sequential form takes it -- only the fill differs --; the look-ahead pass and
                                     //!< lockstep sets have no weighted fill
  bool correlated_constraints = false;   //!< the Gaussian constraints are tied by a correlation matrix: every sequential
                                        //!< form takes its whitening matrix in the step end; never LOOKAHEAD or LOCKSTEP
};
/** The form of the walk's steps, from the flags alone.  LOOKAHEAD is a candidate: two questions to the device (does the
 *  plan stream codes, is the pass offered for this shape) may still narrow it to CONSUMING, see narrowed(). */
struct WalkForm {
  enum Step {
    REFERENCE,   //!< the reference's launches: per-evaluator evaluation (when systematics float), event chunks, step end
    BATCHED,     //!< one group evaluation fused with the event sum, then the step end
    CONSUMING,   //!< the group's fused step, which also clears histograms and normalisations for the next one
    LOCKSTEP,    //!< the consuming step, launched by the chain's lockstep set for all its chains
    LOOKAHEAD,   //!< the consuming step over a pair of evaluator sets: one or two steps per pass
    MIXED        //!< kernel-density members evaluated on the walk's stream, the histogram members in their group, the
                 //!< event sum over both kinds of column: the per-evaluator chain bit for bit, no host wait between steps
  } step;
  bool batched;      //!< the group is bound, tuned and asked for step-end time-outs (also where nothing is re-evaluated)
  bool reevaluate;
  unsigned gsteps;   //!< steps (LOOKAHEAD: passes) per recorded graph; 0: nothing is recorded
  bool adapts_fill_form() const { return step == BATCHED || step == CONSUMING || (step == MIXED && batched); }
  WalkForm narrowed() const { return WalkForm{CONSUMING, batched, reevaluate, gsteps}; }
};
inline WalkForm choose_form(const WalkFlags& f) {
  // a fit with kernel-density members: one form whether or not systematics float (lockstep sets and the look-ahead pass
  // are not offered with such members); its steps are recorded like the batched forms'
  if (f.mixed && !f.reference_form) return WalkForm{WalkForm::MIXED, f.has_group, f.systematics_float, f.graph_steps};
  if (f.mixed) return WalkForm{WalkForm::REFERENCE, false, f.systematics_float, 0};
  const bool batched = f.has_group && !f.reference_form;
  const bool fused = batched && f.systematics_float;
  WalkForm::Step step = WalkForm::REFERENCE;
  if (fused && !f.consume) step = WalkForm::BATCHED;
  if (fused && f.consume) {
    // (a correlated proposal, weighted events, weighted Monte Carlo samples, correlated constraints: asked with lookahead,
    // or given a lockstep set, the walk goes sequentially)
    step = (f.covariance_proposal || f.event_weights || f.sample_weights || f.correlated_constraints)
               ? WalkForm::CONSUMING
           : f.in_lockstep_set   ? WalkForm::LOCKSTEP
           : (f.lookahead_asked && !f.lut_output && f.nparameters <= 256) ? WalkForm::LOOKAHEAD
                                                                           : WalkForm::CONSUMING;
  }
  // recorded steps need the batched form; a lockstep chain's steps are recorded by its set
  return WalkForm{step, batched, f.systematics_float, (fused && step != WalkForm::LOCKSTEP) ? f.graph_steps : 0};
}

/** The same for a walk whose proposal is named apart from its other facts (mcmc.h: the proposal is the walk's, the rest
 *  are the chain's). */
inline WalkForm choose_form(bool covariance_proposal, WalkFlags f) {
  f.covariance_proposal = covariance_proposal;
  return choose_form(f);
}
/** ... and whose data events carry weights (the data's, named beside the proposal). */
inline WalkForm choose_form(bool covariance_proposal, bool event_weights, WalkFlags f) {
  f.event_weights = event_weights;
  return choose_form(covariance_proposal, f);
}
/** ... and whose histogram members carry sample multiplicities (the signals', named beside the data's weights). */
inline WalkForm choose_form(bool covariance_proposal, bool event_weights, bool sample_weights, WalkFlags f) {
  f.sample_weights = sample_weights;
  return choose_form(covariance_proposal, event_weights, f);
}
/** ... and whose constraints are correlated (the walk's, named beside the signals' weights). */
inline WalkForm choose_form(bool covariance_proposal, bool event_weights, bool sample_weights, bool correlated_constraints,
                            WalkFlags f) {
  f.correlated_constraints = correlated_constraints;
  return choose_form(covariance_proposal, event_weights, sample_weights, f);
}

}  // namespace sxmc
