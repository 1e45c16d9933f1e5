// hip_block_shim/hip/hip_runtime.h -- TEST INFRASTRUCTURE: the few HIP names hdlc_repair.hip uses, for a CPU build that
// runs one workgroup at a time with a std::thread per lane (tests/c/repair_kernel_main.cpp).  __shared__ becomes a static
// (one block at a time), __syncthreads() a barrier over the block, __ballot() an exchange over the wave's 64 threads.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <barrier>
#include <atomic>
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(...)
#define __forceinline__ inline
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
typedef void *hipStream_t;
typedef void *hipEvent_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
inline hipError_t hipGetLastError() { return hipSuccess; }
struct Idx { unsigned x; };
extern thread_local Idx threadIdx;
extern Idx blockIdx;
extern std::barrier<> *g_block_barrier;
extern std::barrier<> *g_wave_barrier[4];
extern unsigned char g_pred[256];
inline void __syncthreads() { g_block_barrier->arrive_and_wait(); }
inline unsigned long long __ballot(bool p)
{
    const unsigned t = threadIdx.x, w = t >> 6;
    g_pred[t] = p;
    g_wave_barrier[w]->arrive_and_wait();
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) m |= (unsigned long long) g_pred[w * 64 + l] << l;
    g_wave_barrier[w]->arrive_and_wait();
    return m;
}
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int atomicAdd(int32_t *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
#define hipLaunchKernelGGL(...) ((void) 0)
