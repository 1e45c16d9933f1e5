// channeliser_body.h -- what the channeliser's kernels are made of and the launch that picks among them, shared by
// channeliser.hip (int16 input, GNUAIS_FMT_CS16) and channeliser_fmt.hip (the other sample formats); the kernels' own
// text is channeliser_kernels.inc.  The only places the format acts are wide_load<F>(), where a wide sample is read, and
// wide_word<F>(), where it becomes the (I lo, Q hi) int16 word of the definition (wide_format.h); everything behind that load is one text for
// all formats.  The forms themselves are described at the top of channeliser.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "wide_format.h"

namespace gnuais {
namespace {

typedef short short2_t __attribute__((ext_vector_type(2)));
struct alignas(4) float_pair { float i, q; };      // a cf32 pair: 4-byte aligned, read with one 8-byte load

__device__ __forceinline__ int sat16(int x) { return min(max(x, -32768), 32767); }
__device__ __forceinline__ int lo16(uint32_t w) { return (int) (int16_t) (w & 0xffffu); }
__device__ __forceinline__ int hi16(uint32_t w) { return (int) (int16_t) (w >> 16); }

// mixed sample of wide word x at mixer word cs = (C lo, S hi): (mr, mi) = x * e^{-j theta}, rounded, saturated
__device__ __forceinline__ void mix(uint32_t x, uint32_t cs, int &mr, int &mi)
{
    const int I = lo16(x), Q = hi16(x), C = lo16(cs), S = hi16(cs);
    const int u = I * C + Q * S;
    const int v = Q * C - I * S;
    mr = sat16((u + 16384) >> 15);
    mi = sat16((v + 16384) >> 15);
}

__device__ __forceinline__ uint32_t pack2(int a, int b) { return (uint32_t) (uint16_t) a | ((uint32_t) (uint16_t) b << 16); }

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, a), __builtin_bit_cast(short2_t, b), c, false);
}

// What a lane holds of one wide sample between its load and its use: the bits as they were loaded -- from the call's
// input in format F (native: a = the int16 word, the 8-bit pair or I's fp32 bits, b = Q's fp32 bits) or from the carry
// (a = the converted word) -- so that the conversion can wait until the value is needed.  Converting inside the branch
// that loads would put a wait for the load there, and a pair's two loads would no longer be in flight together.
struct WideRaw { uint32_t a, b; bool native; };

// pair i of the call's input in format F: 4, 2, 2 or 8 bytes per lane, contiguous over a wave
template <int F>
__device__ __forceinline__ WideRaw wide_load(const void *in, size_t i)
{
    if constexpr (F == FMT_CS16) {
        return {static_cast<const uint32_t *>(in)[i], 0u, true};
    } else if constexpr (F == FMT_CF32) {
        const float_pair x = static_cast<const float_pair *>(in)[i];
        return {__builtin_bit_cast(uint32_t, x.i), __builtin_bit_cast(uint32_t, x.q), true};
    } else {
        return {static_cast<const uint16_t *>(in)[i], 0u, true};
    }
}

// the definition's (I lo, Q hi) int16 word of what was loaded (wide_format.h)
template <int F>
__device__ __forceinline__ uint32_t wide_word(const WideRaw &r)
{
    if constexpr (F == FMT_CS16) return r.a;
    else if constexpr (F == FMT_CF32)
        return r.native ? wide_word_cf32(__builtin_bit_cast(float, r.a), __builtin_bit_cast(float, r.b)) : r.a;
    else return r.native ? (F == FMT_CU8 ? wide_word_cu8(r.a) : wide_word_cs8(r.a)) : r.a;
}

// the wide sample of stream s at call index t: the call's input, the carry before it (converted words), zero before that
template <int F>
__device__ __forceinline__ WideRaw wide_raw_at(const void *__restrict__ in, const uint32_t *__restrict__ hist, int M, int T,
                                               int t, int s)
{
    if (t >= 0) return wide_load<F>(in, (size_t) t * M + s);
    if (t >= -(T - 1)) return {hist[(size_t) (T - 1 + t) * M + s], 0u, false};
    return {0u, 0u, false};
}

// The fast form's pair of samples t, t + 1 (`two`: the second one exists).  For the converted formats the common case,
// both from the call's input, issues its two loads back to back in one block, so that one wait serves both; left to the
// two separate branches of wide_raw_at(), the second load waited for the first.  The int16 kernels keep the plain path
// (and with it their instruction streams).
template <int F>
__device__ __forceinline__ void wide_pair_at(const void *__restrict__ in, const uint32_t *__restrict__ hist, int M, int T,
                                             int t, int s, bool two, WideRaw &w0, WideRaw &w1)
{
    if constexpr (F != FMT_CS16) {
        if (t >= 0 && two) {
            w0 = wide_load<F>(in, (size_t) t * M + s);
            w1 = wide_load<F>(in, (size_t) (t + 1) * M + s);
            return;
        }
    }
    w0 = wide_raw_at<F>(in, hist, M, T, t, s);
    w1 = two ? wide_raw_at<F>(in, hist, M, T, t + 1, s) : WideRaw{0u, 0u, false};
}

template <int F>
__device__ __forceinline__ uint32_t wide_at(const void *__restrict__ in, const uint32_t *__restrict__ hist, int M, int T,
                                            int t, int s)
{
    return wide_word<F>(wide_raw_at<F>(in, hist, M, T, t, s));
}

__device__ __forceinline__ int phase_at(int ph0, int t, int P)
{
    int p = (int) (((long long) ph0 + t) % P);
    return p < 0 ? p + P : p;
}

template <int K> struct OutVec;
template <> struct OutVec<1> { using T = uint32_t; __device__ static T make(const uint32_t *w) { return w[0]; } };
template <> struct OutVec<2> { using T = uint2; __device__ static T make(const uint32_t *w) { return make_uint2(w[0], w[1]); } };
template <> struct OutVec<3> { using T = uint3; __device__ static T make(const uint32_t *w) { return make_uint3(w[0], w[1], w[2]); } };
template <> struct OutVec<4> { using T = uint4; __device__ static T make(const uint32_t *w) { return make_uint4(w[0], w[1], w[2], w[3]); } };

template <class Kernels, int K>
hipError_t launch_chan_k(const ChanLaunch &a, dim3 grid, hipStream_t stream)
{
    switch (a.NA) {
    case 4: Kernels::template fast<K, 4>(a, grid, stream); break;
    case 8: Kernels::template fast<K, 8>(a, grid, stream); break;
    case 17: Kernels::template fast<K, 17>(a, grid, stream); break;
    case 33:
        if constexpr (K <= 2) { Kernels::template fast<K, 33>(a, grid, stream); break; }
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
    return hipSuccess;
}

// The launch for one format's kernels.  Kernels: fast<K, NA>(a, grid, stream), direct(a, grid, stream) and
// carry(grid, stream, in, hist_in, hist_out, M, T, len) launch that format's instances.
template <class Kernels>
hipError_t launch_chan_with(const ChanLaunch &a0, uint32_t *hist_out, hipStream_t stream)
{
    ChanLaunch a = a0;
    if (a.M <= 0 || a.K <= 0 || a.K > CHAN_MAX_K || a.D <= 0 || a.len <= 0 || a.len % a.D || a.T < 1) return hipErrorInvalidValue;
    const int rows = a.len / a.D;
    a.n_groups = (a.M + 63) / 64;
    // segments: enough waves to fill the chip (about 4096), no shorter than 128 rows (the halo is NA-1 groups)
    long long want = ((long long) rows * a.n_groups + 4095) / 4096;
    a.seg_rows = (int) std::min<long long>(2048, std::max<long long>(128, want));
    const long long n_seg = (rows + a.seg_rows - 1) / a.seg_rows;
    const long long blocks = n_seg * a.n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (a.NA > 0) {
        const dim3 grid((unsigned) blocks);
        switch (a.K) {
        case 1: e = launch_chan_k<Kernels, 1>(a, grid, stream); break;
        case 2: e = launch_chan_k<Kernels, 2>(a, grid, stream); break;
        case 3: e = launch_chan_k<Kernels, 3>(a, grid, stream); break;
        case 4: e = launch_chan_k<Kernels, 4>(a, grid, stream); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        Kernels::direct(a, dim3((unsigned) blocks, (unsigned) a.K), stream);
    }
    if (e != hipSuccess) return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.T > 1) {
        const long long n = (long long) (a.T - 1) * a.M;
        Kernels::carry(dim3((unsigned) ((n + 255) / 256)), stream, a.in, a.hist, hist_out, a.M, a.T, a.len);
    }
    return hipGetLastError();
}

} // namespace
} // namespace gnuais
