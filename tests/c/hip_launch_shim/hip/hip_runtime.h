// hip_launch_shim/hip/hip_runtime.h -- TEST INFRASTRUCTURE: the HIP names nmea_device.hip uses, for a CPU build in which
// a launch really runs (tests/c/message_kernel_main.cpp): a std::thread per lane, the blocks of the grid one after the
// other, __syncthreads() a barrier over the block, __shared__ a static (one block at a time).  A kernel may leave early
// only with its whole block.  rocPRIM's entry points are stood in for beside this file and in ../hip_serial_shim.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <barrier>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
typedef void *hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyDeviceToHost = 2 };
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
struct Idx { unsigned x; };
extern thread_local Idx threadIdx, blockIdx;
extern Idx gridDim;
extern std::barrier<> *g_block_barrier;
extern std::vector<size_t> g_dynamic_lds;   // the dynamic shared memory every launch asked for: the program checks its arrays against it
inline void __syncthreads() { g_block_barrier->arrive_and_wait(); }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
// the wave exchange of chunk_scan_kernel, which this build never launches (the chunk-table path stays with the GPU tests)
inline uint32_t __shfl_up(uint32_t, int) { abort(); }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class T> inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
template <class T> inline T atomicCAS(T *p, T expect, T v)
{
    __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
    return expect;
}
template <class T> inline T atomicMax(T *p, T v)
{
    T o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) { }
    return o;
}
template <class K, class... A> inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t dynamic_lds, hipStream_t, A... args)
{
    std::barrier<> bar((ptrdiff_t) block.x);
    g_block_barrier = &bar;
    g_dynamic_lds.push_back(dynamic_lds);
    gridDim.x = grid.x;
    std::vector<std::thread> lanes;
    for (unsigned t = 0; t < block.x; ++t)
        lanes.emplace_back([&, t] {
            threadIdx.x = t;
            for (unsigned b = 0; b < grid.x; ++b) {
                blockIdx.x = b;
                kernel(args...);
                bar.arrive_and_wait();          // the next block reuses the statics
            }
        });
    for (auto &l : lanes) l.join();
}
