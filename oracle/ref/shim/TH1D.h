// Stand-in for ROOT's TH1D header: the class lives in TH1.h, as in ROOT.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_TH1D_H
#define ORACLE_REF_SHIM_TH1D_H
#include <TH1.h>
#endif
