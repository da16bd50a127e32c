// Stand-in for ROOT's TH3D (see TH1.h).  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_TH3D_H
#define ORACLE_REF_SHIM_TH3D_H
#include <TH1.h>
class TH3D : public TH1 {
 public:
  TH3D(const char*, const char*, int, double, double, int, double, double, int, double, double) {
    shim_no_root("TH3D");
  }
  void GetRandom3(double&, double&, double&) { shim_no_root("TH3D::GetRandom3"); }
  static TClass* Class() { shim_no_root("TH3D::Class"); }
};
#endif
