// Host-only stand-in for the hemi portability macros: the CPU mode that the fitted code selects
// with -DHEMI_CUDA_DISABLE, where a "kernel" is a plain function run once over the whole range.
// Written from the call sites in the two translation units this recipe compiles; test
// infrastructure only (oracle/ref/README.md).
#ifndef ORACLE_REF_SHIM_HEMI_H
#define ORACLE_REF_SHIM_HEMI_H

#ifndef HEMI_CUDA_DISABLE
#error "this stand-in only spells hemi's CPU mode: compile with -DHEMI_CUDA_DISABLE"
#endif
// HEMI_DEV_CODE stays undefined: every #ifdef HEMI_DEV_CODE picks its host branch.

#define HEMI_KERNEL(name) void name
#define HEMI_KERNEL_NAME(name) name
#define HEMI_KERNEL_LAUNCH(name, grid, block, shared_bytes, stream, ...) name(__VA_ARGS__)
#define HEMI_DEV_CALLABLE
#define HEMI_DEV_CALLABLE_INLINE inline
#define HEMI_DEV_CALLABLE_MEMBER
#define HEMI_DEV_CALLABLE_INLINE_MEMBER inline

inline int hemiGetElementOffset() { return 0; }
inline int hemiGetElementStride() { return 1; }

#endif
