// sxmc_multigroup.cpp -- several chains over the same tables in one pass (lockstep sets) and the look-ahead pass of one chain.
#include "sxmc_host.h"

using namespace sxhost;

namespace sxhost {
// Can this launch keep several histograms per member in LDS (the chains of a lockstep set, the look-ahead pass)?  With
// the histogram in LDS, a program that runs as straight-line code, and rows, a bucketed or an ordered table.
static bool lockstep_class_ok(const LaunchClass& c) {
  const int form = c.shape.form;
  return c.shape.lds_hist && c.prog_simple && (form == kFormRows || form == kFormBucketed || form == kFormOrdered) &&
         (c.shape.nobs != 0 || form == kFormOrdered);
}

// Chains can share a fill pass when their launch plans are the same plan over the same tables.
bool multigroup_prepare(sxmc_multigroup* mg) {
  const size_t C = mg->groups.size();
  sxmc_group* g0 = mg->groups[0];
  mg->why_not.clear();
  for (size_t c = 1; c < C; c++) {
    sxmc_group* g = mg->groups[c];
    if (g->members.size() != g0->members.size() || g->plan.classes.size() != g0->plan.classes.size()) {
      mg->why_not = "the chains' groups differ in members or launches";
      return false;
    }
    for (size_t j = 0; j < g->members.size(); j++) {
      if (g->members[j]->store != g0->members[j]->store || g->members[j]->nbins != g0->members[j]->nbins ||
          g->members[j]->lower != g0->members[j]->lower || g->members[j]->upper != g0->members[j]->upper) {
        mg->why_not = "the chains' evaluators do not share their sample tables (sxmc_hist_create_shared) or geometry";
        return false;
      }
    }
  }
  DeviceProps props;
  if (get_props(props)) return false;
  mg->fill_fn.assign(g0->plan.classes.size(), nullptr);
  mg->lds_bytes.assign(g0->plan.classes.size(), 0);
  mg->fill_w.assign(g0->plan.classes.size(), 0u);
  for (size_t i = 0; i < g0->plan.classes.size(); i++) {
    const LaunchClass& c0 = g0->plan.classes[i];
    if (!lockstep_class_ok(c0)) {
      mg->why_not = "a launch of the plan has its histogram beyond LDS, a run-time decoded program or a pre-binned column";
      return false;
    }
    for (size_t c = 1; c < C; c++) {
      const LaunchClass& cc = mg->groups[c]->plan.classes[i];
      if (cc.shape.nobs != c0.shape.nobs || cc.shape.nslot != c0.shape.nslot || cc.shape.lds_hist != c0.shape.lds_hist ||
          cc.shape.form != c0.shape.form || cc.prog != c0.prog || cc.prog_simple != c0.prog_simple ||
          cc.shape.grid != c0.shape.grid || cc.shape.threads != c0.shape.threads || cc.member_idx != c0.member_idx ||
          cc.partition != c0.partition) {
        mg->why_not = "the chains' launch plans differ (systematics, launch configuration)";
        return false;
      }
    }
    const bool ordered = c0.shape.form == kFormOrdered;
    size_t hist_words = 0, lds = 0;   // the kernel's `w` argument and its LDS, for C chains
    if (!ordered) {
      hist_words = sx_fill_w(c0.shape);   // (one chain's histogram words: C of them between header and trash words)
      lds = (4 + C * hist_words + 64) * 4;
    } else {
      // ordered fill: the kernel argument is the replica layout; as many replicas as fit beside the other chains'
      // (codes: the padded form of the histograms if the chains' histograms fit that way with the smallest queues; a plan
      // with two workgroups per CU leaves each of them half the CU's LDS)
      sxplan::OrderedLdsIn in;
      in.max_bins = c0.max_bins;
      in.nchain = (int)C;
      in.padded_rstride = c0.padded_rstride;
      in.codes = c0.codes;   // (the queues of ambiguous rows, fill_ordered_body's CODES, are shared by the chains)
      const size_t per_cu = (size_t)std::max(1, c0.shape.grid / std::max(1, props.cus));
      in.share = (size_t)props.lds_per_cu / std::min<size_t>(per_cu, 2);
      in.queue_cap = g0->plan_cfg.queue_log;
      const sxplan::OrderedLds o = sxplan::ordered_lds_layout(in);
      lds = o.bytes;
      hist_words = o.word;
    }
    if (lds > (size_t)props.lds_per_cu) {
      mg->why_not = "the chains' histograms do not fit LDS together";
      return false;
    }
    SxRtcSpec k{};
    k.nobs = c0.shape.nobs;
    k.nslot = c0.shape.nslot;
    k.lds_hist = 1;
    k.form = c0.shape.form;
    k.nchain = (int)C;
    // (ordered tables: the kernel is compiled for the workgroup size of the plan -- 512, 768 or 1024 lanes)
    k.max_threads = ordered ? (c0.shape.threads <= 512 ? 512 : c0.shape.threads <= 768 ? 768 : 1024) : 0;
    k.nops = (int)c0.prog.size();
    for (size_t q = 0; q < c0.prog.size(); q++) k.ops[q] = c0.prog[q];
    std::string err;
    mg->fill_fn[i] = sx_rtc_get(k, &err);
    if (!mg->fill_fn[i]) {
      mg->why_not = "the lockstep kernel could not be compiled: " + err.substr(0, 300);
      return false;
    }
    mg->lds_bytes[i] = lds;
    mg->fill_w[i] = (unsigned)hist_words;
  }
  return true;
}
}  // namespace sxhost

extern "C" {

int sxmc_multigroup_create(const sxmc_group_t* groups, int ngroups, sxmc_multigroup_t* out) {
  SX_REQUIRE(groups && out && ngroups >= 2 && ngroups <= 4, "a multigroup steps 2 to 4 chains together");
  for (int i = 0; i < ngroups; i++) SX_REQUIRE(groups[i], "null group");
  sxmc_multigroup* mg = new sxmc_multigroup;
  mg->groups.assign(groups, groups + ngroups);
  if (const char* e = measure_env("SXMC_JOINT_STEP_END")) mg->joint_ends = std::atoi(e) != 0;   // (A/B runs of whole programs)
  *out = mg;
  return SXMC_OK;
}

int sxmc_multigroup_destroy(sxmc_multigroup_t mg) {
  delete mg;
  return SXMC_OK;
}

int sxmc_multigroup_step_async(sxmc_multigroup_t mg, sxmc_stream_t s, const sxmc_step_args* args) {
  SX_FLUSH();
  SX_ORDER(s);
  TraceRange trace("sxmc: lockstep step (one fill pass for the set's chains + their step ends)");
  SX_REQUIRE(mg && args, "null argument");
  hipStream_t st = (hipStream_t)s;
  const size_t C = mg->groups.size();
  for (const sxmc_group* g : mg->groups) {
    if (g->proposal_factor) {
      return fail(SXMC_ERR_STATE, "a member group has a proposal factor set: lockstep sets have no correlated step end "
                                  "-- step the chains one by one (sxmc_group_step_async)");
    }
    if (!g->event_weights.empty()) {
      return fail(SXMC_ERR_STATE, "a member group has event weights set: lockstep sets have no weighted step end "
                                  "-- step the chains one by one (sxmc_group_step_async)");
    }
    if (weighted_members(g)) {
      return fail(SXMC_ERR_STATE, "a member group has sample multiplicities set: lockstep sets have no weighted fill "
                                  "-- step the chains one by one (sxmc_group_step_async)");
    }
  }
  for (const sxmc_group* g : mg->groups) {
    if (g->constraint_whitening) {
      return fail(SXMC_ERR_STATE, "a member group has a constraint whitening matrix set: lockstep sets have no step end "
                                  "with correlated constraints -- step the chains one by one (sxmc_group_step_async)");
    }
  }
  // every chain's own plan first (may upload: before anything is launched)
  bool replan = mg->seen.size() != C;
  for (size_t c = 0; c < C; c++) {
    sxmc_group* g = mg->groups[c];
    const sxmc_step_args& a = args[c];
    SX_REQUIRE(a.d_means && a.d_sigmas && a.d_rng && a.d_nll_current && a.d_nll_proposed && a.d_v_current &&
                   a.d_v_proposed && a.d_accepted && a.d_counter && a.d_jump_buffer && a.d_jump_width &&
                   a.d_nexpected && a.d_n_mc && a.d_source_id && a.d_norms && a.nparameters > 0,
               "null argument");
    g->plan_cfg.box = 0;   // (several chains per pass: the ordered form; the boxed one has no such kernel)
    int rc = group_refresh(g);
    if (rc) return rc;
    if (!replan && mg->seen[c] != g->plan_generation) replan = true;
    rc = group_check_bound(g, true);
    if (rc) return rc;
    if (!g->same_points) return fail(SXMC_ERR_STATE, "members do not share one set of evaluation points");
    if (!g->cfg_lut) {
      rc = ensure_event_classes(g, false);
      if (rc) return rc;
    }
    note_stepping(g);
    g->last_stream = st;
  }
  if (replan) {
    if (t_capturing) return fail(SXMC_ERR_STATE, "the chains' plans are out of date: step once before recording a graph");
    mg->seen.resize(C);
    for (size_t c = 0; c < C; c++) mg->seen[c] = mg->groups[c]->plan_generation;
    if (!multigroup_prepare(mg)) {
      mg->seen.clear();
      return fail(SXMC_ERR_STATE, "these chains cannot share a fill pass: " + mg->why_not);
    }
  }
  for (size_t c = 0; c < C; c++) {
    sxmc_group* g = mg->groups[c];
    const bool zero_launched = g->prezeroed != 1;
    int rc = group_prepare_fill(g, st, false);
    if (rc) return rc;
    g->last_step_launches = zero_launched ? 1 : 0;
  }
  // ONE pass over the tables for all chains
  sxmc_group* g0 = mg->groups[0];
  for (size_t i = 0; i < g0->plan.classes.size(); i++) {
    const LaunchClass& c0 = g0->plan.classes[i];
    if (c0.shape.grid <= 0) continue;
    SxChainDescsHost ch{};
    for (size_t c = 0; c < C; c++) ch.d[c] = mg->groups[c]->plan.classes[i].d_descs.get();
    const bool rec = g0->prof && !t_capturing && g0->prof_n < (int)g0->ev0.size();
    SX_HIP(sx_rtc_launch_multi(mg->fill_fn[i], c0.shape.grid, c0.shape.threads, mg->lds_bytes[i], ch, c0.d_segs.get(),
                               c0.d_blk_off.get(), mg->fill_w[i], (unsigned)mg->groups[0]->debug_mode, st,
                               rec ? (void*)g0->ev0[g0->prof_n] : nullptr, rec ? (void*)g0->ev1[g0->prof_n] : nullptr));
    if (rec) g0->prof_n++;
  }
  // every chain's own step end -- in two launches for the whole set where every chain's end has the two-launch form
  // (the chains then pay the kernels' latency once, not C times), else chain by chain
  bool joint = mg->joint_ends;
  for (size_t c = 0; c < C && joint; c++) {
    const sxmc_group* g = mg->groups[c];
    joint = g->max_bins == g0->max_bins &&
            !step_end_takes_tail(g, false, step_rows(g, false).ne);
  }
  SxChainEnds ends{};
  for (size_t c = 0; c < C; c++) {
    sxmc_group* g = mg->groups[c];
    const sxmc_step_args& p = args[c];
    g->last_step_launches += (int)g0->plan.classes.size();
    const StepRows rows = step_rows(g, false);   // (ensure_event_classes: in the first loop, before anything was launched)
    const SxStepArgs a = sx_step_args(p, g->members.size());
    if (joint) {
      SxChainEnd& e = ends.c[c];
      e.lookup_descs = rows.descs;
      e.hist_descs = g->d_descs.get();
      e.nrows = rows.ne;
      e.weight = rows.weight;
      e.sums = g->d_step_sums.get();
      e.ticket = g->d_ticket.get() + sxstep::kTicket;
      e.nblocks = (unsigned)step_sum_blocks(rows.ne);
      e.a = a;
      g->last_step_launches += 2;
      mark_cleared(g, false);
      continue;
    }
    int rc = group_step_tail(g, st, false, rows, a);
    if (rc) return rc;
  }
  if (joint) SX_HIP(sx_launch_chain_ends(ends, (int)C, (int)g0->members.size(), g0->max_bins, 128, st));
  return SXMC_OK;
}

int sxmc_multigroup_set_joint_step_end(sxmc_multigroup_t mg, int enable) {
  SX_REQUIRE(mg, "null multigroup");
  mg->joint_ends = enable != 0;
  return SXMC_OK;
}

// The look-ahead walk's pass (see finish2_zero_kernel): groups[0] evaluates the step's proposal (its evaluators are
// bound to a->d_v_proposed / a->d_norms), groups[1] the look-ahead vector (bound to d_v_lookahead / d_norms_lookahead).
int sxmc_multigroup_lookahead_step_async(sxmc_multigroup_t mg, sxmc_stream_t s, const sxmc_step_args* a,
                                         double* d_v_lookahead, const unsigned* d_norms_lookahead, const int* d_cap) {
  SX_FLUSH();
  SX_ORDER(s);
  TraceRange trace("sxmc: look-ahead pass (two evaluations, one or two steps)");
  SX_REQUIRE(mg && a && d_v_lookahead && d_norms_lookahead, "null argument");
  SX_REQUIRE(mg->groups.size() == 2, "the look-ahead walk steps exactly two groups: the proposal's and the look-ahead's");
  SX_REQUIRE(a->d_means && a->d_sigmas && a->d_rng && a->d_nll_current && a->d_nll_proposed && a->d_v_current &&
                 a->d_v_proposed && a->d_accepted && a->d_counter && a->d_jump_buffer && a->d_jump_width &&
                 a->d_nexpected && a->d_n_mc && a->d_source_id && a->d_norms && a->nparameters > 0,
             "null argument");
  SX_REQUIRE(a->nparameters <= 256, "the look-ahead walk stages its vectors in LDS: at most 256 parameters");
  for (const sxmc_group* g : mg->groups) {
    if (g->proposal_factor) {
      return fail(SXMC_ERR_STATE, "a member group has a proposal factor set: the look-ahead pass has no correlated form "
                                  "-- walk sequentially (sxmc_group_lookahead_supported says so beforehand)");
    }
    if (!g->event_weights.empty()) {
      return fail(SXMC_ERR_STATE, "a member group has event weights set: the look-ahead pass has no weighted form "
                                  "-- walk sequentially (sxmc_group_lookahead_supported says so beforehand)");
    }
    if (weighted_members(g)) {
      return fail(SXMC_ERR_STATE, "a member group has sample multiplicities set: the look-ahead pass has no weighted fill "
                                  "-- walk sequentially (sxmc_group_lookahead_supported says so beforehand)");
    }
  }
  for (const sxmc_group* g : mg->groups) {
    if (g->constraint_whitening) {
      return fail(SXMC_ERR_STATE, "a member group has a constraint whitening matrix set: the look-ahead pass has no form "
                                  "with correlated constraints -- walk sequentially (sxmc_group_lookahead_supported "
                                  "says so beforehand)");
    }
  }
  hipStream_t st = (hipStream_t)s;
  bool replan = mg->seen.size() != 2;
  for (size_t c = 0; c < 2; c++) {
    sxmc_group* g = mg->groups[c];
    g->plan_cfg.box = 0;   // (several chains per pass: the ordered form; the boxed one has no such kernel)
    int rc = group_refresh(g);
    if (rc) return rc;
    if (!replan && mg->seen[c] != g->plan_generation) replan = true;
    rc = group_check_bound(g, true);
    if (rc) return rc;
    if (!g->same_points) return fail(SXMC_ERR_STATE, "members do not share one set of evaluation points");
    if (g->cfg_lut) return fail(SXMC_ERR_STATE, "the look-ahead walk sums over event classes: switch the lookup table off");
    if (g->sparse_ready && g->cfg_sparse) return fail(SXMC_ERR_STATE, "the look-ahead walk needs histograms that fit LDS");
    rc = ensure_event_classes(g, false);
    if (rc) return rc;
    note_stepping(g);
    g->last_stream = st;
  }
  sxmc_group *ga = mg->groups[0], *gb = mg->groups[1];
  SX_REQUIRE(ga->members.size() == gb->members.size() && ga->members.size() <= 1024 && ga->ec[0].K == gb->ec[0].K,
             "the two groups must hold the same members over the same data");
  if (step_end_takes_tail(ga, false, ga->ec[0].K)) {
    return fail(SXMC_ERR_STATE,
                "the look-ahead walk is not offered for this shape: the sequential step ends in the one-workgroup form "
                "(at most 256 look-ups), which the pass has no counterpart of -- walk sequentially "
                "(sxmc_group_lookahead_supported says so beforehand)");
  }
  if (replan) {
    if (t_capturing) return fail(SXMC_ERR_STATE, "the chains' plans are out of date: step once before recording a graph");
    mg->seen.resize(2);
    for (size_t c = 0; c < 2; c++) mg->seen[c] = mg->groups[c]->plan_generation;
    if (!multigroup_prepare(mg)) {
      mg->seen.clear();
      return fail(SXMC_ERR_STATE, "these groups cannot share a fill pass: " + mg->why_not);
    }
  }
  for (size_t c = 0; c < 2; c++) {
    sxmc_group* g = mg->groups[c];
    const bool zero_launched = g->prezeroed != 1;
    int rc = group_prepare_fill(g, st, false);
    if (rc) return rc;
    g->last_step_launches = zero_launched ? 1 : 0;
  }
  for (size_t i = 0; i < ga->plan.classes.size(); i++) {
    const LaunchClass& c0 = ga->plan.classes[i];
    if (c0.shape.grid <= 0) continue;
    SxChainDescsHost ch{};
    ch.d[0] = ga->plan.classes[i].d_descs.get();
    ch.d[1] = gb->plan.classes[i].d_descs.get();
    const bool rec = ga->prof && !t_capturing && ga->prof_n < (int)ga->ev0.size();
    SX_HIP(sx_rtc_launch_multi(mg->fill_fn[i], c0.shape.grid, c0.shape.threads, mg->lds_bytes[i], ch, c0.d_segs.get(),
                               c0.d_blk_off.get(), mg->fill_w[i], (unsigned)mg->groups[0]->debug_mode, st,
                               rec ? (void*)ga->ev0[ga->prof_n] : nullptr, rec ? (void*)ga->ev1[ga->prof_n] : nullptr));
    if (rec) ga->prof_n++;
  }
  const sxmc_group::EventClasses &ea = ga->ec[0], &eb = gb->ec[0];
  const unsigned long long ne = ea.K;
  const int block = (int)sxstep::kStepSumRows;
  // each candidate's event sum is cut exactly like the sequential step's (group_step_tail): the same blocks of 128
  // rows, the same cap, so the partial sums and their reduction round identically
  const int half = step_sum_blocks(ne);
  const SxStepArgs k = sx_step_args(*a, ga->members.size());
  // the pass's step end: ONE cooperative launch where both candidates' event sums fit 128 lanes of a finisher
  // (step_end2_kernel; the same switch as the sequential step's), else lookup + event sums, then step end + clearing
  const bool coop = 2 * half <= kCoopMaxWorkers && step_end_is_cooperative(ga, ne);
  if (coop) {
    SX_HIP(sx_launch_step_end2(ea.d_descs.get(), eb.d_descs.get(), ga->d_descs.get(), gb->d_descs.get(), (int)ga->members.size(),
                               std::max(ga->max_bins, gb->max_bins), ne, ea.d_weight.get(), eb.d_weight.get(), ga->d_coop_slots.get(),
                               ga->d_coop_last.get(), ga->d_ticket.get(), half, d_norms_lookahead, d_v_lookahead, d_cap, k, st));
  } else {
    SX_HIP(sx_launch_eval_nll2(ea.d_descs.get(), eb.d_descs.get(), (int)ga->members.size(), ne, ea.d_weight.get(), eb.d_weight.get(),
                               a->d_v_proposed, d_v_lookahead, a->d_nexpected, a->d_n_mc, a->d_source_id, a->d_norms,
                               d_norms_lookahead, ga->d_step_sums.get(), gb->d_step_sums.get(), half, block, st));
    SX_HIP(sx_launch_finish2_zero(ga->d_descs.get(), gb->d_descs.get(), (int)ga->members.size(), std::max(ga->max_bins, gb->max_bins),
                                  (size_t)half, ga->d_step_sums.get(), gb->d_step_sums.get(), d_norms_lookahead, d_v_lookahead, d_cap, k,
                                  128, st));
  }
  for (size_t c = 0; c < 2; c++) {
    sxmc_group* g = mg->groups[c];
    g->last_step_launches += (int)ga->plan.classes.size() + (coop ? 1 : 2);
    mark_cleared(g, false);
  }
  return SXMC_OK;
}

int sxmc_group_lookahead_supported(sxmc_group_t g, int* ok) {
  SX_REQUIRE(g && ok, "null argument");
  *ok = 0;
  if (g->proposal_factor) return SXMC_OK;   // (no correlated look-ahead pass; asked before the group is touched)
  if (g->constraint_whitening) return SXMC_OK;   // (nor one with correlated constraints)
  if (!g->event_weights.empty()) return SXMC_OK;   // (nor a weighted one)
  if (weighted_members(g)) return SXMC_OK;         // (nor one over sample multiplicities)
  g->plan_cfg.box = 0;  // (the pass runs over the ordered form; the question could be asked of g->ordered and leave the setting alone)
  int rc = group_refresh(g);
  if (rc) return rc;
  if (!g->same_points || g->cfg_lut || (g->sparse_ready && g->cfg_sparse) || g->members.empty()) return SXMC_OK;
  if (!g->members[0]->has_points) return SXMC_OK;
  rc = ensure_event_classes(g, false);
  if (rc) return rc;
  if (step_end_takes_tail(g, false, g->ec[0].K)) return SXMC_OK;
  // the pass keeps TWO histograms per member in LDS (the proposal's and the look-ahead's): what multigroup_prepare
  // will require of every launch of the plan
  DeviceProps props;
  if (get_props(props)) return SXMC_OK;
  for (const LaunchClass& c : g->plan.classes) {
    if (!lockstep_class_ok(c)) return SXMC_OK;
    // one histogram's words: an ordered table's `w` is the layout word, whose low 24 bits are the words between replicas
    const unsigned w = sx_fill_w(c.shape);
    const size_t words = c.shape.form == kFormOrdered ? (w & 0xFFFFFFu) : w;
    if ((4 + 2 * words + 64) * 4 > (size_t)props.lds_per_cu) return SXMC_OK;
  }
  *ok = 1;
  return SXMC_OK;
}

// The first look-ahead vector of a walk: what the step after the pending one would propose if the pending one
// were rejected (current vector + jump width x the deviates that step end will draw; generators untouched).
int sxmc_lookahead_begin(sxmc_stream_t s, int nparameters, const sxmc_rng_state* d_rng, const float* d_jump_width,
                         const double* d_v_current, double* d_v_lookahead) {
  SX_FLUSH();
  SX_ORDER(s);
  SX_REQUIRE(d_rng && d_jump_width && d_v_current && d_v_lookahead && nparameters > 0, "null argument");
  SX_HIP(sx_launch_peek_next_proposal(nparameters, d_rng, d_jump_width, d_v_current, d_v_lookahead, (hipStream_t)s));
  return SXMC_OK;
}

}  // extern "C"
