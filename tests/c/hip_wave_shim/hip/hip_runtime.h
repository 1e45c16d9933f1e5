// hip_wave_shim/hip/hip_runtime.h -- TEST INFRASTRUCTURE: tests/c/hip_block_shim's names and what a lane-per-channel
// walk such as hdlc_long.hip uses on top of them (tests/c/long_kernel_main.cpp): blockDim, the wave vote __any(), the
// bit-count builtins, and dynamic shared memory as an ordinary array that the program defines (one block at a time).
#pragma once
#include "../../hip_block_shim/hip/hip_runtime.h"
#undef __shared__
#define __shared__
extern Idx blockDim;
inline int __any(int p) { return __ballot(p != 0) != 0; }
inline int __ffs(int v) { return __builtin_ffs(v); }
inline int __clz(int v) { return v ? __builtin_clz((unsigned) v) : 32; }
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
