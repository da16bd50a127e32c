// test_mixed_plan.cpp -- what a MIXED walk (histogram + kernel-density signals in one recordable step) decides and
// refuses without a device: the form of the steps (sxmc_amd/include/sxmc/walk_plan.h: choose_form) over every
// combination of the flags, with the new flag set and clear; the column table of sxmc_group_set_columns
// (sxmc_amd/csrc/sxmc_plan.h: columns_error, the rule the entry point applies); and the null-handle answers of the new
// entry points of include/sxmc_hip.h.  Links libsxmc_hip.so and calls nothing in it that touches a device.  Run by
// tests/test_mixed_plan_cpu.py.
#include <sxmc_hip.h>

#include <string>
#include <vector>

#include "../../sxmc_amd/csrc/sxmc_plan.h"
#include "../../sxmc_amd/include/sxmc/walk_plan.h"
#include "mini_test.h"

using sxmc::WalkFlags;
using sxmc::WalkForm;

template <typename F>
static void for_every_flag_set(F body) {
  for (unsigned bits = 0; bits < 128; bits++)
    for (size_t nparameters : {5u, 256u, 257u})
      for (unsigned graph_steps : {0u, 8u, 16u}) {
        WalkFlags f{(bits & 1) != 0,  (bits & 2) != 0,  (bits & 4) != 0, (bits & 8) != 0,
                    (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0, nparameters, graph_steps};
        body(f);
      }
}

TEST(ChooseForm, MixedUnlessTheReferenceFormIsAsked) {
  for_every_flag_set([](WalkFlags f) {
    f.mixed = true;
    const WalkForm w = sxmc::choose_form(f);
    if (f.reference_form) {
      EXPECT_TRUE(w.step == WalkForm::REFERENCE);
      EXPECT_EQ(w.gsteps, 0u);
      EXPECT_TRUE(!w.batched);
      EXPECT_TRUE(!w.adapts_fill_form());
    } else {
      EXPECT_TRUE(w.step == WalkForm::MIXED);     // whether or not systematics float, whatever else was asked
      EXPECT_EQ(w.gsteps, f.graph_steps);         // its steps are recorded as asked
      EXPECT_EQ(w.batched, f.has_group);          // the group: the histogram members, where there are any
      EXPECT_EQ(w.adapts_fill_form(), f.has_group);
    }
    EXPECT_EQ(w.reevaluate, f.systematics_float);
  });
}

TEST(ChooseForm, UnchangedWithTheFlagClear) {
  // the booleans as the walk derived them before there was a mixed form (tests/cpp/test_walk_plan.cpp has the same)
  for_every_flag_set([](WalkFlags f) {
    EXPECT_TRUE(!f.mixed);   // the default of the trailing member
    const WalkForm w = sxmc::choose_form(f);
    const bool batched = f.has_group && !f.reference_form;
    const bool reevaluate = f.systematics_float;
    const bool in_lockstep = f.in_lockstep_set && batched && reevaluate && f.consume;
    const unsigned gsteps = (batched && reevaluate && !in_lockstep) ? f.graph_steps : 0;
    const bool ahead = f.lookahead_asked && batched && reevaluate && f.consume && !in_lockstep && !f.lut_output &&
                       f.nparameters <= 256;
    const bool sequential = !in_lockstep && !ahead;
    EXPECT_EQ(w.batched, batched);
    EXPECT_EQ(w.reevaluate, reevaluate);
    EXPECT_EQ(w.gsteps, gsteps);
    EXPECT_TRUE(w.step != WalkForm::MIXED);
    EXPECT_EQ(w.step == WalkForm::LOCKSTEP, in_lockstep);
    EXPECT_EQ(w.step == WalkForm::LOOKAHEAD, ahead);
    EXPECT_EQ(w.step == WalkForm::CONSUMING, sequential && batched && reevaluate && f.consume);
    EXPECT_EQ(w.step == WalkForm::BATCHED, sequential && batched && reevaluate && !f.consume);
    EXPECT_EQ(w.step == WalkForm::REFERENCE, !(batched && reevaluate));
    EXPECT_EQ(w.adapts_fill_form(), batched && reevaluate && !in_lockstep && !ahead);
  });
}

TEST(ChooseForm, TheStepsKeepTheirNumbers) {
  // (MIXED is appended: what was compiled against the earlier values keeps its meaning)
  EXPECT_EQ((int)WalkForm::REFERENCE, 0);
  EXPECT_EQ((int)WalkForm::BATCHED, 1);
  EXPECT_EQ((int)WalkForm::CONSUMING, 2);
  EXPECT_EQ((int)WalkForm::LOCKSTEP, 3);
  EXPECT_EQ((int)WalkForm::LOOKAHEAD, 4);
  EXPECT_EQ((int)WalkForm::MIXED, 5);
}

TEST(Columns, EveryMemberExactlyOnce) {
  const int ok3[] = {-1, 0, -1, 1, 2};
  EXPECT_TRUE(sxplan::columns_error(3, 5, ok3) == nullptr);
  const int ok_order[] = {2, 0, 1};   // (members need not come in their own order)
  EXPECT_TRUE(sxplan::columns_error(3, 3, ok_order) == nullptr);
  const int dense_only[] = {-1, -1};
  EXPECT_TRUE(sxplan::columns_error(0, 2, dense_only) == nullptr);
  const int repeats[] = {0, 1, 1, -1};
  EXPECT_TRUE(std::string(sxplan::columns_error(2, 4, repeats)).find("two columns") != std::string::npos);
  const int omits[] = {0, -1, 2};
  EXPECT_TRUE(std::string(sxplan::columns_error(3, 3, omits)).find("no column") != std::string::npos);
  const int beyond[] = {0, 1, 2};
  EXPECT_TRUE(sxplan::columns_error(2, 3, beyond) != nullptr);
  const int below[] = {0, -2};
  EXPECT_TRUE(sxplan::columns_error(1, 2, below) != nullptr);
  EXPECT_TRUE(sxplan::columns_error(1, 0, ok3) != nullptr);
  EXPECT_TRUE(sxplan::columns_error(1, 1, nullptr) != nullptr);
  // every table over two members and up to four columns: valid exactly when each member is named once
  for (int n = 1; n <= 4; n++) {
    std::vector<int> t((size_t)n, -1);
    for (;;) {
      int count[2] = {0, 0};
      for (int v : t)
        if (v >= 0) count[v]++;
      EXPECT_EQ(sxplan::columns_error(2, n, t.data()) == nullptr, count[0] == 1 && count[1] == 1);
      int q = 0;
      while (q < n && t[(size_t)q] == 1) t[(size_t)q++] = -1;
      if (q == n) break;
      t[(size_t)q]++;
    }
  }
}

TEST(Entries, NullHandlesAreInvalidArguments) {
  const int one[] = {-1};
  EXPECT_EQ(sxmc_group_set_columns(nullptr, 1, one), SXMC_ERR_INVALID);
  EXPECT_TRUE(std::string(sxmc_last_error()).find("null group") != std::string::npos);
  EXPECT_EQ(sxmc_group_eval_columns_nll_async(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, 64, 256),
            SXMC_ERR_INVALID);
  EXPECT_EQ(sxmc_group_finish_columns_step_async(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, 0),
            SXMC_ERR_INVALID);
  EXPECT_EQ(sxmc_kde_eval_on_stream_async(nullptr, 1, nullptr), SXMC_ERR_INVALID);
  short pars[4];
  size_t n = 0;
  unsigned long long count = 0;
  EXPECT_EQ(sxmc_kde_parameters_read(nullptr, pars, 4, &n), SXMC_ERR_INVALID);
  EXPECT_EQ(sxmc_kde_evaluation_count(nullptr, &count), SXMC_ERR_INVALID);
}

int main(int argc, char** argv) { return mini::run_all(argc > 1 ? argv[1] : nullptr); }
