// hip_serial_shim/hip/hip_runtime.h -- TEST INFRASTRUCTURE: the few HIP names frame_unique.hip uses, for a CPU build
// (tests/c/unique_kernel_main.cpp).  Its kernels have no barrier and no LDS, so a launch is a loop: block after block,
// lane after lane.  rocPRIM's two entry points are stood in for beside this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#define __global__
#define __device__
#define __host__
#define __restrict__
#define __launch_bounds__(...)
#define __forceinline__ inline
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
typedef void *hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
struct Idx { unsigned x; };
extern Idx threadIdx, blockIdx, gridDim;
template <class T> inline T atomicAdd(T *p, T v) { const T o = *p; *p = o + v; return o; }
template <class T> inline T atomicMin(T *p, T v) { const T o = *p; if (v < o) *p = v; return o; }
template <class K, class... A> inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t, hipStream_t, A... args)
{
    gridDim.x = grid.x;
    for (unsigned b = 0; b < grid.x; ++b)
        for (unsigned t = 0; t < block.x; ++t) {
            blockIdx.x = b;
            threadIdx.x = t;
            kernel(args...);
        }
}
