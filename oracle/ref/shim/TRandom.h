// Stand-in for ROOT's TRandom whose global generator is a SCRIPTED stream: Uniform() and
// Gaus(mean, sigma) pop the next value of a queue that the driver fills from the case file, and
// every call is logged as (kind, arguments), so a recorded run shows how many draws a step
// takes, of which kind and in which order.  Gaus(m, s) returns m + s * z in double with z popped
// from the queue: that arithmetic is this stand-in's, not ROOT's.  Popping an empty queue is an
// error that ends the program.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_TRANDOM_H
#define ORACLE_REF_SHIM_TRANDOM_H

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

struct ShimRandomCall {
  int kind;       // 0 = Uniform(), 1 = Gaus(mean, sigma)
  double a, b;    // Gaus: mean, sigma; Uniform: 0, 0
  double popped;  // the scripted value the call consumed
};

class TRandom {
 public:
  std::deque<double> queue;
  std::vector<ShimRandomCall> log;

  double Uniform() {
    double u = pop("Uniform");
    log.push_back({0, 0.0, 0.0, u});
    return u;
  }
  double Gaus(double mean = 0, double sigma = 1) {
    double z = pop("Gaus");
    log.push_back({1, mean, sigma, z});
    return mean + sigma * z;
  }
  long Poisson(double) {
    std::fprintf(stderr, "oracle/ref shim: TRandom::Poisson is not scripted\n");
    std::abort();
  }

 private:
  double pop(const char* who) {
    if (queue.empty()) {
      std::fprintf(stderr, "oracle/ref shim: %s() on an empty scripted queue\n", who);
      std::exit(3);
    }
    double v = queue.front();
    queue.pop_front();
    return v;
  }
};

inline TRandom shim_random;
inline TRandom* gRandom = &shim_random;

#endif
