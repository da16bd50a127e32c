// test_walk_plan.cpp -- the schedule of sxmc::MCMC's walk (sxmc_amd/include/sxmc/walk_plan.h), device-free: the rules
// the walk takes from that header, swept by brute force against the expressions of the walk they were cut out of
// (written out literally here) and against what a schedule must satisfy whatever its numbers.  No HIP, no library;
// a plain build and one under ASan + UBSan (Makefile: test_walk_plan, test_walk_plan_asan), run by
// tests/test_walk_plan_cpu.py.
//
// test_walk_plan --dump nsteps burnin_steps sync_interval adapt_interval two_forms: the steps after which the jump
// buffer is read back, on one line, for comparison with sxmc_amd.mcmc.flush_due.
#include <cstdlib>
#include <set>

#include "../../sxmc_amd/include/sxmc/walk_plan.h"
#include "mini_test.h"

using sxmc::WalkSchedule;

static const unsigned SYNCS[] = {1, 2, 7, 16, 100};
static const unsigned ADAPTS[] = {0, 1, 5, 1000};

/** every schedule of the sweep: nsteps 0..70, burnin_steps 0..nsteps, the intervals above, both values of two_forms */
template <typename F>
static void for_every_schedule(F body) {
  for (unsigned nsteps = 0; nsteps <= 70; nsteps++)
    for (unsigned burnin = 0; burnin <= nsteps; burnin++)
      for (unsigned sync : SYNCS)
        for (unsigned adapt : ADAPTS)
          for (int two = 0; two < 2; two++) body(WalkSchedule{nsteps, burnin, sync, adapt}, two != 0);
}

TEST(WalkSchedule, FlushDueIsTheWalksOwnExpression) {
  for_every_schedule([](const WalkSchedule& s, bool two_forms) {
    const unsigned nsteps = s.nsteps, burnin_steps = s.burnin_steps, sync_interval = s.sync_interval,
                   adapt_interval = s.adapt_interval;
    for (unsigned i = 0; i < nsteps; i++) {
      const bool want = i % sync_interval == 0 || i == nsteps - 1 || i == burnin_steps - 1 ||
                        i == 2 * burnin_steps - 1 ||
                        (two_forms && adapt_interval > 0 && i % adapt_interval == adapt_interval - 1);
      EXPECT_EQ(s.flush_due(i, two_forms), want);
    }
  });
}

TEST(WalkSchedule, RunsTileTheWalkAndEndOnTheOnlyDueStepTheyHold) {
  for_every_schedule([](const WalkSchedule& s, bool two_forms) {
    unsigned covered = 0, i = 0;
    while (i < s.nsteps) {
      const unsigned f = s.run_end(i, two_forms);
      EXPECT_TRUE(f >= i && f < s.nsteps);
      EXPECT_TRUE(s.flush_due(f, two_forms));
      for (unsigned j = i; j < f; j++) EXPECT_TRUE(!s.flush_due(j, two_forms));
      covered += f - i + 1;
      i = f + 1;   // (the next run starts where this one ended: no gap, no overlap)
    }
    EXPECT_EQ(i, s.nsteps);       // with nsteps == 0 nothing runs
    EXPECT_EQ(covered, s.nsteps);
  });
}

TEST(WalkSchedule, EveryRetuningStepStartsARun) {
  for_every_schedule([](const WalkSchedule& s, bool two_forms) {
    std::set<unsigned> starts;
    for (unsigned i = 0; i < s.nsteps; i = s.run_end(i, two_forms) + 1) starts.insert(i);
    for (unsigned i = 0; i < s.nsteps; i++) {
      EXPECT_EQ(s.retune_due(i), i == s.burnin_steps || i == 2 * s.burnin_steps);
      if (s.retune_due(i)) EXPECT_TRUE(starts.count(i) == 1);
    }
    // without a burn-in the unsigned terms burnin_steps - 1 and 2 * burnin_steps - 1 match no step, and step 0 re-tunes
    if (s.burnin_steps == 0 && s.nsteps > 0) EXPECT_TRUE(s.retune_due(0));
  });
}

TEST(SplitRun, ReplaysOnlyAfterTheFirstRunAndOnlyWholeGraphs) {
  for (unsigned n = 0; n <= 120; n++)
    for (unsigned gs = 0; gs <= 13; gs++)
      for (int first = 0; first < 2; first++) {
        const sxmc::RunSplit r = sxmc::split_run(n, gs, first != 0);
        EXPECT_EQ(r.replays * gs + r.remainder, n);
        if (first || gs == 0 || n < gs) EXPECT_EQ(r.replays, 0u);
        // the walk's own rule: replay = gsteps > 0 && i > 0 && n >= gsteps; then n / gsteps replays, n % gsteps steps
        const bool replay = gs > 0 && !first && n >= gs;
        EXPECT_EQ(r.replays, replay ? n / gs : 0u);
        EXPECT_EQ(r.remainder, replay ? n % gs : n);
        if (r.replays > 0) EXPECT_TRUE(r.remainder < gs);
      }
}

TEST(LookaheadRound, PassCountsAreTheWalksOwnArithmetic) {
  // (steps, passes) seen so far: below the 16-pass threshold, at it, beyond it; rates below 1, near 1.75, capped at 2
  const struct {
    double steps;
    size_t passes;
  } seen[] = {{0, 0}, {20, 15}, {40, 15}, {20, 16}, {16, 16}, {28, 16}, {40, 17}, {1000, 400}, {1700, 1000}, {5, 16}};
  const unsigned graphs[] = {0, 1, 6, 8, 50, 399, 400};
  for (const auto& sn : seen)
    for (unsigned gsteps : graphs)
      for (int have = 0; have < 2; have++)
        for (unsigned need = 1; need <= 400; need++) {
          const sxmc::LookaheadRound r = sxmc::lookahead_round(need, sn.steps, sn.passes, gsteps, have != 0);
          // the walk as it was written: ahead_passes_seen, ahead_steps_seen, graph
          const double ahead_steps_seen = sn.steps;
          const size_t ahead_passes_seen = sn.passes;
          const bool graph = have != 0;
          const double rate =
              ahead_passes_seen >= 16 ? std::min(2.0, 1.03 * ahead_steps_seen / ahead_passes_seen) : 1.75;
          unsigned k = std::max(1u, (unsigned)(need / rate));
          const unsigned k0 = k;
          const bool records = gsteps > 0 && k > gsteps && !graph;
          unsigned eager = 0, replays = 0;
          if (gsteps > 0 && k > gsteps) {
            if (!graph) {
              eager = 1;   // one_pass(): plans in place before recording
              k--;
            }
            replays = k / gsteps;
            k %= gsteps;
          }
          EXPECT_EQ(r.records, records);
          EXPECT_EQ(r.records ? 1u : 0u, eager);
          EXPECT_EQ(r.replays, replays);
          EXPECT_EQ(r.single_passes, k);
          // whatever the numbers: at least one pass, all k0 of them accounted for, a recording only where it may be
          EXPECT_TRUE((r.records ? 1u : 0u) + r.replays * gsteps + r.single_passes >= 1);
          EXPECT_EQ((r.records ? 1u : 0u) + r.replays * gsteps + r.single_passes, k0);
          EXPECT_EQ(r.records, gsteps > 0 && !have && k0 > gsteps);
          if (r.records) EXPECT_TRUE(r.replays >= 1);   // what is recorded is replayed at once
          if (gsteps == 0) EXPECT_EQ(r.replays, 0u);
        }
}

TEST(ChooseForm, IsTheWalksOwnBooleans) {
  // every combination of the flags against the booleans as the walk derived them
  for (unsigned bits = 0; bits < 128; bits++)
    for (size_t nparameters : {5u, 256u, 257u})
      for (unsigned graph_steps : {0u, 8u}) {
        const bool has_group = bits & 1, reference_form = bits & 2, floats = bits & 4, consume = bits & 8;
        const bool lut_output = bits & 16, lockstep = bits & 32, asked = bits & 64;
        const sxmc::WalkForm w = sxmc::choose_form(
            sxmc::WalkFlags{has_group, reference_form, floats, consume, lut_output, lockstep, asked, nparameters, graph_steps});
        const bool batched = has_group && !reference_form;
        const bool reevaluate = floats;
        const bool in_lockstep = lockstep && batched && reevaluate && consume;
        const unsigned gsteps = (batched && reevaluate && !in_lockstep) ? graph_steps : 0;
        const bool ahead = asked && batched && reevaluate && consume && !in_lockstep && !lut_output && nparameters <= 256;
        EXPECT_EQ(w.batched, batched);
        EXPECT_EQ(w.reevaluate, reevaluate);
        EXPECT_EQ(w.gsteps, gsteps);
        EXPECT_EQ(w.step == sxmc::WalkForm::LOCKSTEP, in_lockstep);
        EXPECT_EQ(w.step == sxmc::WalkForm::LOOKAHEAD, ahead);
        // the step the sequential walk launches: the fused one, the group evaluation, or the reference's launches
        const bool sequential = !in_lockstep && !ahead;
        EXPECT_EQ(w.step == sxmc::WalkForm::CONSUMING, sequential && batched && reevaluate && consume);
        EXPECT_EQ(w.step == sxmc::WalkForm::BATCHED, sequential && batched && reevaluate && !consume);
        EXPECT_EQ(w.step == sxmc::WalkForm::REFERENCE, !(batched && reevaluate));
        EXPECT_EQ(w.adapts_fill_form(), batched && reevaluate && !in_lockstep && !ahead);
        const sxmc::WalkForm n = w.narrowed();   // a look-ahead candidate the device turned down
        EXPECT_TRUE(n.step == sxmc::WalkForm::CONSUMING && n.gsteps == w.gsteps && n.batched == w.batched);
      }
}

int main(int argc, char** argv) {
  if (argc == 7 && std::string(argv[1]) == "--dump") {
    const WalkSchedule s{(unsigned)std::atoi(argv[2]), (unsigned)std::atoi(argv[3]), (unsigned)std::atoi(argv[4]),
                         (unsigned)std::atoi(argv[5])};
    const bool two_forms = std::atoi(argv[6]) != 0;
    for (unsigned i = 0; i < s.nsteps; i++)
      if (s.flush_due(i, two_forms)) std::printf("%u ", i);
    std::printf("\n");
    return 0;
  }
  return mini::run_all(argc > 1 ? argv[1] : nullptr);
}
