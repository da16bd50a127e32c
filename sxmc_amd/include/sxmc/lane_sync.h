// lane_sync.h -- where the host threads of the ensemble runners meet: the lanes of ensemble_concurrent (experiment.h)
// at a LaneBarrier, the rank threads of ensemble_multi_gpu (multi_gpu.h) at a Rendezvous.  The standard library only:
// tests/cpp/test_ensemble_plan.cpp runs both without a device.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <mutex>

namespace sxmc {

/** Where the lanes of ensemble_concurrent meet, twice per round of experiments: when every lane's walk is set up (before
 *  any of them queues its first long run of steps) and when every lane's last step has finished (before any tears
 *  down).  Set-up and tear-down synchronise the whole device; beside a chain that has a second of graph replays queued
 *  each of those calls waits that second out, under the set-up lock the other lanes need -- which is how eight lanes came
 *  to walk one at a time at 1e5 steps per experiment.  A lane that fails breaks the barrier: nobody waits for it. */
class LaneBarrier {
 public:
  void arrive_and_wait(size_t expected) {
    std::unique_lock<std::mutex> lk(m);
    if (broken) return;
    const unsigned long long gen = generation;
    if (++count >= expected) {
      count = 0;
      generation++;
      cv.notify_all();
      return;
    }
    cv.wait(lk, [&] { return generation != gen || broken; });
  }
  void break_all() {
    std::lock_guard<std::mutex> lk(m);
    broken = true;
    cv.notify_all();
  }

 private:
  std::mutex m;
  std::condition_variable cv;
  size_t count = 0;
  unsigned long long generation = 0;
  bool broken = false;
};

/** How the device threads of ensemble_multi_gpu meet before the collective: every thread arrives exactly once, with
 *  "my part went well" or not, and all of them learn whether EVERY part went well.  A collective is entered by all
 *  ranks or by none -- a rank that failed on the way must never leave its peers waiting inside ncclAllGather. */
class Rendezvous {
 public:
  explicit Rendezvous(size_t n_) : n(n_) {}
  bool arrive(bool ok) {
    std::unique_lock<std::mutex> lock(m);
    all_ok = all_ok && ok;
    if (++arrived == n) {
      cv.notify_all();
    } else {
      cv.wait(lock, [&] { return arrived == n; });
    }
    return all_ok;
  }

 private:
  std::mutex m;
  std::condition_variable cv;
  size_t n, arrived = 0;
  bool all_ok = true;
};

}  // namespace sxmc
