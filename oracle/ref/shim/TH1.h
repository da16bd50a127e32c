// Stand-in for ROOT's histogram classes (as in ROOT, TH1.h also declares TH1D): enough for the histogram-export and sampling members of
// the compiled translation unit to compile and link.  The driver never calls those members, so
// everything that would need ROOT aborts.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_TH1_H
#define ORACLE_REF_SHIM_TH1_H

#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>

[[noreturn]] inline void shim_no_root(const char* what) {
  std::fprintf(stderr, "oracle/ref shim: %s needs ROOT, which this build does not have\n", what);
  std::abort();
}

class TClass {};

class TH1 {
 public:
  virtual ~TH1() {}
  virtual void Sumw2() { shim_no_root("TH1::Sumw2"); }
  virtual int GetBin(int, int = 0, int = 0) const { shim_no_root("TH1::GetBin"); }
  virtual void SetBinContent(int, double) { shim_no_root("TH1::SetBinContent"); }
  virtual void SetBinError(int, double) { shim_no_root("TH1::SetBinError"); }
  virtual double GetRandom() const { shim_no_root("TH1::GetRandom"); }
  virtual TClass* IsA() const { shim_no_root("TH1::IsA"); }
  virtual const char* ClassName() const { return "TH1"; }
  static TClass* Class() { shim_no_root("TH1::Class"); }
};

class TH1D : public TH1 {
 public:
  TH1D(const char*, const char*, int, double, double) { shim_no_root("TH1D"); }
  static TClass* Class() { shim_no_root("TH1D::Class"); }
};

#endif
