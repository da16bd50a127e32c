// Stand-in for CUDA's math_constants.h on a host-only build.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_MATH_CONSTANTS_H
#define ORACLE_REF_SHIM_MATH_CONSTANTS_H
#include <math.h>
#define CUDART_INF_F ((float)INFINITY)
#define CUDART_NAN_F ((float)NAN)
#define CUDART_INF ((double)INFINITY)
#define CUDART_NAN ((double)NAN)
#define CUDART_PI 3.1415926535897931e+0
#define CUDART_PI_F 3.141592654f
#endif
