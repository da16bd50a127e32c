// Stand-in for ROOT's TStopwatch: the launch-shape tuner that uses it is compiled out on the host.
#ifndef ORACLE_REF_SHIM_TSTOPWATCH_H
#define ORACLE_REF_SHIM_TSTOPWATCH_H
class TStopwatch {
 public:
  void Start(bool = true) {}
  void Stop() {}
  double RealTime() { return 0.0; }
};
#endif
