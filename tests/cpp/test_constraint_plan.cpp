// test_constraint_plan.cpp -- correlated constraints in the walk's plan (sxmc_amd/include/sxmc/walk_plan.h), device-free: over
// every combination of the facts a walk is planned from, a walk with correlated_constraints never takes the look-ahead pass or a
// lockstep set's step and is otherwise planned like the same walk asked without either; and without the fact choose_form
// answers what it answers for the same flags built without naming it.  No HIP, no library; plain and under ASan + UBSan
// (constraints.mk), run by tests/test_constraint_whitening_cpu.py.
#include "../../sxmc_amd/include/sxmc/walk_plan.h"
#include "mini_test.h"

using sxmc::WalkFlags;
using sxmc::WalkForm;

static bool same(const WalkForm& a, const WalkForm& b) {
  return a.step == b.step && a.batched == b.batched && a.reevaluate == b.reevaluate && a.gsteps == b.gsteps;
}

/** every combination: nine booleans, the vector lengths on each side of 256, recorded steps or none */
template <typename F>
static void for_every_walk(F body) {
  const size_t lengths[] = {1, 15, 256, 257};
  const unsigned graphs[] = {0, 16};
  for (unsigned bits = 0; bits < (1u << 9); bits++)
    for (size_t np : lengths)
      for (unsigned g : graphs) {
        WalkFlags f{(bits & 1) != 0,  (bits & 2) != 0,  (bits & 4) != 0, (bits & 8) != 0,   (bits & 16) != 0,
                    (bits & 32) != 0, (bits & 64) != 0, np,              g,                 (bits & 128) != 0,
                    (bits & 256) != 0};
        body(f);
      }
}

TEST(ConstraintPlan, TheFactIsOffByDefaultAndTheSweepReachesBothForms) {
  size_t lookaheads = 0, locksteps = 0;
  for_every_walk([&](const WalkFlags& f) {
    EXPECT_TRUE(!f.correlated_constraints);
    const WalkForm got = sxmc::choose_form(f);
    lookaheads += got.step == WalkForm::LOOKAHEAD;
    locksteps += got.step == WalkForm::LOCKSTEP;
  });
  EXPECT_TRUE(lookaheads > 0 && locksteps > 0);
}

TEST(ConstraintPlan, CorrelatedConstraintsNeverYieldLookaheadOrLockstep) {
  size_t narrowed = 0;
  for_every_walk([&](WalkFlags f) {
    const WalkForm plain = sxmc::choose_form(f);
    f.correlated_constraints = true;
    const WalkForm got = sxmc::choose_form(f);
    EXPECT_TRUE(got.step != WalkForm::LOOKAHEAD && got.step != WalkForm::LOCKSTEP);
    // ... and is the plan of the same walk asked without a lockstep set and without lookahead
    WalkFlags alone = f;
    alone.correlated_constraints = false;
    alone.in_lockstep_set = false;
    alone.lookahead_asked = false;
    EXPECT_TRUE(same(got, sxmc::choose_form(alone)));
    if (plain.step == WalkForm::LOOKAHEAD || plain.step == WalkForm::LOCKSTEP) {
      narrowed++;
      EXPECT_TRUE(got.step == WalkForm::CONSUMING);
    } else {
      EXPECT_TRUE(same(got, plain));   // every sequential form takes them as it is
    }
  });
  EXPECT_TRUE(narrowed > 0);
}

int main(int argc, char** argv) { return mini::run_all(argc > 1 ? argv[1] : nullptr); }
