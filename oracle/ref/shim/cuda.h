// Stand-in for the CUDA driver header on a host-only build: a stream type and stream calls that
// do nothing and succeed.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_CUDA_H
#define ORACLE_REF_SHIM_CUDA_H

typedef int cudaError_t;
typedef int cudaStream_t;
#define cudaSuccess 0

inline cudaError_t cudaStreamCreate(cudaStream_t* s) { *s = 0; return cudaSuccess; }
inline cudaError_t cudaStreamDestroy(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t checkCuda(cudaError_t e) { return e; }

#endif
