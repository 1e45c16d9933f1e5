// hip_cpu/hip/hip_runtime.h -- TEST INFRASTRUCTURE: the one stand-in for <hip/hip_runtime.h> behind which g++ compiles a
// kernel file's own text, host half included, for the CPU (tests/c/*_kernel_main.cpp, under ASan + UBSan).  It holds the
// HIP names those files use and no others; rocPRIM's entry points are stood in for beside it.  All its state is here, as
// inline variables: a program includes a kernel file and calls its launch functions, nothing else.
//
// hipLaunchKernelGGL runs the launch, in one of exactly two ways.
//   Threads (the default): the blocks of the grid one after the other, a std::thread per lane of block.x.  One block runs
//     at a time, which is why static __shared__ can be a plain `static`.  __syncthreads() is a barrier over the block;
//     __ballot() and __any() exchange over the lane's own wave of 64 (the last wave may be partial).  Dynamic shared
//     memory is a heap block of exactly the launch's dynamic_lds bytes, 16-byte aligned, made for each block and freed
//     when it ends, so ASan sees the first byte past it and any use of it by a later block or launch; a launch with 0
//     bytes has none (a null pointer).  It starts out filled with 0xa5: LDS is never zero on demand.  A kernel reaches it
//     through HIP's own macro HIP_DYNAMIC_SHARED(type, name), here a handle that reads the running block's pointer where
//     it is used, at namespace scope or inside a function.
//     Early exit: a lane may return at any point.  It drops out of its block's and its wave's barriers, and votes 0 in
//     the ballots of the lanes that go on, as an exited lane does on the device.
//   -DHIP_CPU_SERIAL: a plain loop, block after block and lane after lane, for kernel files with no barrier, no LDS and
//     no wave operation.  Atomic counters then hand out their slots in a fixed order.  __shared__, HIP_DYNAMIC_SHARED,
//     __syncthreads, __ballot and __any do not exist in this mode: a file that uses one does not compile.
// The hip* calls are synchronous memset / memcpy or return hipSuccess.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#define __global__
#define __device__
#define __host__
#define __restrict__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
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
inline thread_local Idx threadIdx;
inline Idx blockIdx, blockDim, gridDim;     // one block at a time: the same for every lane that runs
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __ffs(int v) { return __builtin_ffs(v); }
inline int __clz(int v) { return v ? __builtin_clz((unsigned) v) : 32; }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
// the wave exchange of chunk_scan_kernel, which this build never launches (the chunk-table path stays with the GPU tests)
inline uint32_t __shfl_up(uint32_t, int) { abort(); }
template <class T> inline T atomicAdd(T *p, std::type_identity_t<T> v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class T> inline T atomicOr(T *p, std::type_identity_t<T> v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
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
template <class T> inline T atomicMin(T *p, T v)
{
    T o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) { }
    return o;
}

#ifdef HIP_CPU_SERIAL
template <class K, class... A> inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t, hipStream_t, A... args)
{
    gridDim.x = grid.x;
    blockDim.x = block.x;
    for (unsigned b = 0; b < grid.x; ++b)
        for (unsigned t = 0; t < block.x; ++t) {
            blockIdx.x = b;
            threadIdx.x = t;
            kernel(args...);
        }
}
#else
#include <barrier>
#include <deque>
#include <functional>
#include <optional>
#include <thread>
#include <vector>
namespace hip_cpu {
struct Block {                              // the block that is running
    std::barrier<> all;
    std::deque<std::barrier<>> wave;
    std::vector<unsigned char> pred;        // the lanes' votes
    void *dynamic_lds = nullptr;
    Block(unsigned lanes, size_t lds_bytes) : all((ptrdiff_t) lanes), pred(lanes, 0)
    {
        for (unsigned l = 0; l < lanes; l += 64) wave.emplace_back((ptrdiff_t) (lanes - l < 64 ? lanes - l : 64));
        if (lds_bytes && posix_memalign(&dynamic_lds, 16, lds_bytes)) abort();
        if (lds_bytes) memset(dynamic_lds, 0xa5, lds_bytes);
    }
    ~Block() { free(dynamic_lds); }
    void leave(unsigned lane)               // the lane's kernel has returned
    {
        pred[lane] = 0;
        wave[lane >> 6].arrive_and_drop();
        all.arrive_and_drop();
    }
};
inline Block *g_block;
template <class T> struct DynamicShared { operator T *() const { return static_cast<T *>(g_block->dynamic_lds); } };
}
#define __shared__ static
#define HIP_DYNAMIC_SHARED(type, name) static const hip_cpu::DynamicShared<type> name{};
inline void __syncthreads() { hip_cpu::g_block->all.arrive_and_wait(); }
inline unsigned long long __ballot(bool p)
{
    hip_cpu::Block &b = *hip_cpu::g_block;
    const size_t t = threadIdx.x, w = t >> 6, first = w * 64;
    const size_t n = b.pred.size() - first < 64 ? b.pred.size() - first : 64;
    b.pred[t] = p;
    b.wave[w].arrive_and_wait();
    unsigned long long m = 0;
    for (size_t l = 0; l < n; ++l) m |= (unsigned long long) b.pred[first + l] << l;
    b.wave[w].arrive_and_wait();
    return m;
}
inline int __any(int p) { return __ballot(p != 0) != 0; }
namespace hip_cpu {
inline void run_grid(dim3 grid, dim3 block, size_t dynamic_lds, const std::function<void()> &kernel)
{
    gridDim.x = grid.x;
    blockDim.x = block.x;
    if (!grid.x) return;
    // the lanes' threads live as long as the launch (starting one costs more than most kernels' work); when the last
    // lane of a block has returned, that block's shared memory is freed and the next block's made
    std::optional<Block> blk;
    auto open = [&](unsigned b) noexcept {
        g_block = &blk.emplace(block.x, dynamic_lds);
        blockIdx.x = b;
    };
    open(0);
    std::barrier between((ptrdiff_t) block.x, [&]() noexcept { open(blockIdx.x + 1); });
    std::vector<std::thread> lanes;
    for (unsigned t = 0; t < block.x; ++t)
        lanes.emplace_back([&, t] {
            threadIdx.x = t;
            for (unsigned b = 0; b < grid.x; ++b) {
                kernel();
                g_block->leave(t);
                if (b + 1 < grid.x) between.arrive_and_wait();
            }
        });
    for (auto &l : lanes) l.join();
    g_block = nullptr;
}
}
template <class K, class... A> inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t dynamic_lds, hipStream_t, A... args)
{
    hip_cpu::run_grid(grid, block, dynamic_lds, [&] { kernel(args...); });
}
#endif
