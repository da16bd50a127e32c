// Stand-in for ROOT's TMath.h: like the real one, it brings the C math functions into the global
// namespace, which is all the compiled translation units take from it.
#ifndef ORACLE_REF_SHIM_TMATH_H
#define ORACLE_REF_SHIM_TMATH_H
#include <math.h>
#include <cmath>
using std::isnan;
#endif
