// Stand-in for ROOT's TH2D (see TH1.h).  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_TH2D_H
#define ORACLE_REF_SHIM_TH2D_H
#include <TH1.h>
class TH2D : public TH1 {
 public:
  TH2D(const char*, const char*, int, double, double, int, double, double) { shim_no_root("TH2D"); }
  void GetRandom2(double&, double&) { shim_no_root("TH2D::GetRandom2"); }
  static TClass* Class() { shim_no_root("TH2D::Class"); }
};
#endif
