// test_ensemble_plan.cpp -- device-free: how ensemble_multi_gpu shares N experiments of P parameters among G ranks and
// brings their intervals back (sxmc_amd/include/sxmc/ensemble_plan.h), swept over G, N and P; and the meeting points of
// the runners' host threads (lane_sync.h).  No HIP, no library: built plain and under ASan + UBSan by the Makefile, run
// by tests/test_ensemble_plan_cpu.py.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../sxmc_amd/include/sxmc/ensemble_plan.h"
#include "../../sxmc_amd/include/sxmc/intervals.h"
#include "../../sxmc_amd/include/sxmc/lane_sync.h"
#include "mini_test.h"

namespace {

uint32_t bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

/** Experiment k's interval of parameter p: four floats that say where they belong, none of them NaN. */
sxmc::Interval interval_of(size_t k, size_t p) {
  sxmc::Interval iv;
  iv.point_estimate = (float)(1000 * k + 10 * p) + 0.25f;
  iv.lower = iv.point_estimate - 1.5f;
  iv.upper = (float)((k * 7 + p * 3) % 11) - 4.0f;   // (not monotonic in k: the medians have to sort)
  iv.coverage = -999.0f;
  return iv;
}

}  // namespace

TEST(ShardPlan, EveryExperimentHasOneRankAndOneSlot) {
  for (size_t G = 1; G <= 9; G++) {
    for (size_t N = 0; N <= 40; N++) {
      for (size_t P : {(size_t)1, (size_t)5}) {
        const sxmc::ShardPlan plan{G, N, P};
        EXPECT_EQ((N + G - 1) / G, plan.per());
        EXPECT_EQ((size_t)std::ceil((double)N / (double)G) * P * 4, plan.block());
        std::vector<int> owners(N, 0);
        size_t most = 0;
        for (size_t r = 0; r < G; r++) {
          const std::vector<unsigned> ks = plan.experiments_of(r);
          most = std::max(most, ks.size());
          EXPECT_TRUE(ks.size() <= plan.per());
          for (size_t i = 0; i < ks.size(); i++) {
            EXPECT_EQ((unsigned)(r + i * G), ks[i]);   // r, r + G, ...
            EXPECT_TRUE(ks[i] < N);
            owners[ks[i]]++;
            EXPECT_EQ(r, plan.rank_of(ks[i]));
            EXPECT_EQ(i, plan.slot_of(ks[i]));
          }
        }
        for (size_t k = 0; k < N; k++) EXPECT_EQ(1, owners[k]);
        EXPECT_EQ(plan.per(), most);   // (the block is no larger than the fullest rank needs)
      }
    }
  }
}

TEST(ShardPlan, PackThenUnpackReturnsEveryIntervalInExperimentOrder) {
  for (size_t G = 1; G <= 9; G++) {
    for (size_t N = 0; N <= 40; N++) {
      for (size_t P : {(size_t)1, (size_t)5}) {
        const sxmc::ShardPlan plan{G, N, P};
        // every rank packs its own block; the blocks meet rank after rank, as the all-gather leaves them
        std::vector<float> all;
        for (size_t r = 0; r < G; r++) {
          std::vector<float> block = plan.empty_blocks();
          EXPECT_EQ(plan.block(), block.size());
          const std::vector<unsigned> ks = plan.experiments_of(r);
          for (size_t i = 0; i < ks.size(); i++) {
            std::vector<sxmc::Interval> ivs;
            for (size_t p = 0; p < P; p++) ivs.push_back(interval_of(ks[i], p));
            plan.pack(block, i, ivs);
          }
          // slots that no experiment fills stay NaN, the filled ones hold none
          for (size_t j = 0; j < block.size(); j++) EXPECT_EQ(j >= ks.size() * P * 4, std::isnan(block[j]));
          all.insert(all.end(), block.begin(), block.end());
        }
        EXPECT_EQ(G * plan.block(), all.size());
        EXPECT_EQ(all.size(), plan.empty_blocks(G).size());
        const std::vector<float> gathered = plan.unpack(all);
        EXPECT_EQ(N * P * 4, gathered.size());
        for (size_t k = 0; k < N; k++) {
          for (size_t p = 0; p < P; p++) {
            const sxmc::Interval want = interval_of(k, p);
            const float* g = &gathered[(k * P + p) * 4];
            EXPECT_EQ(bits(want.point_estimate), bits(g[0]));
            EXPECT_EQ(bits(want.lower), bits(g[1]));
            EXPECT_EQ(bits(want.upper), bits(g[2]));
            EXPECT_EQ(bits(want.coverage), bits(g[3]));
          }
        }
        for (float v : gathered) EXPECT_TRUE(!std::isnan(v));   // the padding never reaches `gathered`
        // the medians: sxmc::median over the upper limits, 0 without experiments
        const std::vector<float> med = plan.median_upper(gathered, sxmc::median<float>);
        EXPECT_EQ(P, med.size());
        for (size_t p = 0; p < P; p++) {
          std::vector<float> ups;
          for (size_t k = 0; k < N; k++) ups.push_back(interval_of(k, p).upper);
          EXPECT_EQ(bits(N ? sxmc::median(ups) : 0.0f), bits(med[p]));
        }
      }
    }
  }
}

TEST(ShardPlan, AnExperimentWithFewerIntervalsThanParametersLeavesTheRestNaN) {
  const sxmc::ShardPlan plan{2, 3, 5};
  std::vector<float> block = plan.empty_blocks();
  plan.pack(block, 1, std::vector<sxmc::Interval>{interval_of(2, 0), interval_of(2, 1)});
  for (size_t j = 0; j < block.size(); j++) EXPECT_EQ(!(j >= 20 && j < 28), std::isnan(block[j]));
  // ... and one with more than P leaves its neighbour alone
  std::vector<sxmc::Interval> many;
  for (size_t p = 0; p < 9; p++) many.push_back(interval_of(0, p));
  plan.pack(block, 0, many);
  EXPECT_EQ(bits(interval_of(2, 0).point_estimate), bits(block[20]));
  EXPECT_EQ(bits(interval_of(0, 4).coverage), bits(block[19]));
}

TEST(LaneBarrier, RoundsOfUnequalSizeAndABrokenBarrier) {
  // the meeting point of ensemble_concurrent's lanes: every round's participants leave together, a last round with
  // fewer lanes works, and a lane that fails releases everybody for good
  sxmc::LaneBarrier meet;
  const size_t lanes = 4, experiments = 10;     // rounds of 4, 4 and 2
  std::atomic<int> inside{0}, worst{0};
  std::vector<std::thread> threads;
  for (size_t t = 0; t < lanes; t++) {
    threads.emplace_back([&, t]() {
      for (size_t i = t; i < experiments; i += lanes) {
        const size_t round_lanes = std::min(lanes, experiments - (i - t));
        meet.arrive_and_wait(round_lanes);      // "all set up"
        const int now = ++inside;
        int seen = worst.load();
        while (now > seen && !worst.compare_exchange_weak(seen, now)) {
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(2 + (int)t));
        --inside;
        meet.arrive_and_wait(round_lanes);      // "all stepped"
      }
    });
  }
  for (std::thread& th : threads) th.join();
  EXPECT_TRUE(worst.load() >= 2 && worst.load() <= 4);
  // a waiter is released by break_all, and nobody waits afterwards
  std::atomic<bool> released{false};
  std::thread waiter([&]() {
    meet.arrive_and_wait(2);
    released = true;
  });
  std::this_thread::sleep_for(std::chrono::milliseconds(20));
  EXPECT_TRUE(!released.load());
  meet.break_all();
  waiter.join();
  EXPECT_TRUE(released.load());
  meet.arrive_and_wait(5);                       // returns at once
}

TEST(Rendezvous, EveryThreadLearnsWhetherAllWentWell) {
  // the meeting point of ensemble_multi_gpu's rank threads: everybody arrives once; one `false` is everybody's `false`
  for (size_t n : {(size_t)1, (size_t)2, (size_t)8}) {
    for (int failing = -1; failing < (int)n; failing++) {   // -1: nobody fails
      sxmc::Rendezvous meet(n);
      std::vector<int> got(n, -1);
      std::vector<std::thread> threads;
      for (size_t t = 0; t < n; t++) {
        threads.emplace_back([&, t]() {
          std::this_thread::sleep_for(std::chrono::microseconds(200 * ((t * 5) % 3)));   // (arrival order varies)
          got[t] = meet.arrive((int)t != failing) ? 1 : 0;
        });
      }
      for (std::thread& th : threads) th.join();
      for (size_t t = 0; t < n; t++) EXPECT_EQ(failing < 0 ? 1 : 0, got[t]);
    }
  }
}

int main(int argc, char** argv) { return mini::run_all(argc > 1 ? argv[1] : nullptr); }
