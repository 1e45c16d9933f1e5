// wide_kernels.h -- the wide stage's kernels: tune, low-pass and resample wideband (I, Q) streams by U/D into the
// narrowband I/Q the discriminator takes (gnuais_batch_channeliser: U = 1; gnuais_batch_resampler; include/gnuais_hip.h).
// Not part of the reference; all integer, defined exactly in the header and restated in NumPy (tests/chan_ref.py,
// tests/resample_ref.py), so the device matches it bit for bit whatever the order of the sums.  One text for every
// ratio and sample format; channeliser.hip, channeliser_fmt.hip and resampler.hip instantiate it (kernels.h says which
// unit holds what), wide_launch.hip launches it.
//
// Layout: in [len][M] pairs, out [len*U/D][M*K] words, receiver c = s*K + k.  A lane owns one stream and all K offsets:
// it reads each wide sample once, mixes it for every offset, and walks a segment of output rows.  The mixer row, the
// group and its taps depend on the time index alone, which is the same in every lane of a workgroup (lanes are
// streams, the segment is the workgroup's), so they are uniform loads.  Results leave with vector stores only.
//
// Fast form (channeliser_kernel<K, NA, F, RATIONAL>): transposed polyphase over GROUPS (resample_plan.h).  Group g holds the
// wide samples n with g*D <= n*U < (g+1)*D, and each feeds rows g .. g+NA-1 (NA >= ceil(T/D)), whose int32 accumulators
// live in registers; after group g, row g is complete, leaves, and the accumulators shift by one.  Two consecutive
// samples of a group go into one v_dot2c_i32_i16 per accumulator (__builtin_amdgcn_sdot2): the host packed the taps as
// pairs per (pair, accumulator), zero where a tap index is outside [0, T) or the group has an odd last sample.  At an
// integer ratio (RATIONAL = false: U = 1) every group is the D samples from g*D on and reads the same pairs,
// POLY[q][a] = (h[aD + D-1-2q], h[aD + D-2-2q]).  At a rational one a call starts on a period boundary (len is a
// multiple of D, so its rows are a multiple of U): call-local row g = c*U + i has its first sample at c*D + first[i],
// and its size -- floor(D/U) or ceil(D/U) -- and its tap pairs depend on i alone, so the loop carries (c, i) and needs
// no division.  A segment starts NA-1 groups early to fill its accumulators (the halo, ~1 % of a 1500-row segment at
// D = 6); samples before the call come from the carry, before that they are zero.
//
// Direct form (channeliser_direct_kernel<F>): any K and T, one lane per (stream, offset): row m walks the taps j = u_m mod U,
// + U, ... and mixes each sample again.  Used only where the fast form's accumulators do not fit in registers (K > 4, or
// ceil(T/D) above the largest bucket) or the output is not aligned to the fast form's vector store.
//
// The carry (the last H = ceil((T-1)/U) wide samples per stream, converted) is double-buffered: a launch reads one
// buffer and channeliser_carry_kernel<F> writes the other, so no launch reads what it writes.
//
// The only places the format acts are wide_load<F>(), where a wide sample is read, and wide_word<F>(), where it becomes
// the (I lo, Q hi) int16 word of the definition (wide_format.h): 4, 2, 2 or 8 bytes per lane, so no int16 copy of the
// wide stream is ever written, and the carry holds converted words, so calls of different formats may follow each other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>


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

// the wide sample of stream s at call index t: the call's input, the carry before it (converted words; T - 1 = H rows of
// it), zero before that
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

} // namespace

// the fast form.  grid: 1-D, block b = (segment b / n_groups, stream group b % n_groups); 64 threads (one wave),
// thread = one stream.
template <int K, int NA, int F, bool RATIONAL>
__global__ __launch_bounds__(64) void channeliser_kernel(WideLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    // Where the two ratios differ is the group geometry alone, all under RATIONAL.  A few of the arguments are read where
    // each form read them when it had a text of its own -- the carry's rows and the tap pairs before or behind the early
    // return, the pairs per group outside the loop at U = 1 -- which keeps the instruction streams.
    const int U = RATIONAL ? a.U : 1, HR = RATIONAL ? a.H + 1 : 0;
    const int rows = a.len / a.D * U;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const int D = a.D, M = a.M, HT = RATIONAL ? HR : a.T, NP1 = (D + 1) / 2;      // HT - 1: the carry's rows (T - 1 at U = 1)
    const void *__restrict__ in = a.in;
    const uint32_t *__restrict__ hist = a.hist;
    const int32_t *__restrict__ groups = a.groups;
    const uint32_t *__restrict__ pairs = RATIONAL ? a.poly : nullptr;

    // the first group of the segment's halo; at a rational ratio as (period c, phase i), floor division
    const int g0 = r0 - NA + 1;
    int c = 0, i = 0;
    if constexpr (RATIONAL) {
        c = g0 / U, i = g0 % U;
        if (i < 0) { i += U; --c; }
    }

    int p[K];
    {
        const int t_first = RATIONAL ? c * D + groups[3 * i] : g0 * D;
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = phase_at(a.ph0[k], t_first, a.per[k]);
    }

    int acc_r[K][NA], acc_i[K][NA];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < NA; ++j) acc_r[k][j] = acc_i[k][j] = 0;

    const size_t N = (size_t) M * K;
    for (int g = g0; g < r1; ++g) {
        // the group's first sample, its size, its tap pairs (U = 1: the one table, read at its use) and their count
        const int t0 = RATIONAL ? c * D + groups[3 * i] : g * D, size = RATIONAL ? groups[3 * i + 1] : D;
        const uint32_t *hg = RATIONAL ? pairs + (size_t) groups[3 * i + 2] * NA : nullptr;
        const int NP = RATIONAL ? (size + 1) / 2 : NP1;
        for (int q = 0; q < NP; ++q) {
            const int t = t0 + 2 * q;
            const bool two = 2 * q + 1 < size;
            WideRaw w0, w1;                             // both loads first, then the conversions
            wide_pair_at<F>(in, hist, M, HT, t, s, two, w0, w1);
            const uint32_t x0 = wide_word<F>(w0), x1 = wide_word<F>(w1);
            uint32_t pr[K], pi[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t *tab = a.mix + a.off[k];
                int m0r, m0i, m1r = 0, m1i = 0;
                mix(x0, tab[p[k]], m0r, m0i);
                if (++p[k] == a.per[k]) p[k] = 0;
                if (two) {
                    mix(x1, tab[p[k]], m1r, m1i);
                    if (++p[k] == a.per[k]) p[k] = 0;
                }
                pr[k] = pack2(m0r, m1r);
                pi[k] = pack2(m0i, m1i);
            }
            const uint32_t *hp = (RATIONAL ? hg : a.poly) + (size_t) q * NA;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const uint32_t h = hp[j];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    acc_r[k][j] = dot2(pr[k], h, acc_r[k][j]);
                    acc_i[k][j] = dot2(pi[k], h, acc_i[k][j]);
                }
            }
        }
        if (g >= r0) {
            uint32_t w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = pack2(sat16((acc_r[k][0] + 16384) >> 15), sat16((acc_i[k][0] + 16384) >> 15));
            using V = typename OutVec<K>::T;
            *reinterpret_cast<V *>(a.out + (size_t) g * N + (size_t) s * K) = OutVec<K>::make(w);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int j = 0; j + 1 < NA; ++j) {
                acc_r[k][j] = acc_r[k][j + 1];
                acc_i[k][j] = acc_i[k][j + 1];
            }
            acc_r[k][NA - 1] = acc_i[k][NA - 1] = 0;
        }
        if constexpr (RATIONAL)
            if (++i == U) { i = 0; ++c; }
    }
}

// the direct form.  grid: x = (segment, stream group) as above, y = offset k; thread = one stream at offset k.
template <int F>
__global__ __launch_bounds__(64) void channeliser_direct_kernel(WideLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int k = (int) blockIdx.y;
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int U = a.U, D = a.D, M = a.M, T = a.T, HT = a.H + 1, P = a.per[k];
    const int rows = a.len / D * U;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const uint32_t *tab = a.mix + a.off[k];
    for (int m = r0; m < r1; ++m) {
        const long long e = (long long) m * D + D - 1;      // the row's last tick, call-local: the call's sample 0 is tick 0
        int j0 = 0, t = (int) e;                            // U = 1: a tick is a sample (< len), no division
        if (U != 1) {
            j0 = (int) (e % U);
            t = (int) ((e - j0) / U);
        }
        int p = phase_at(a.ph0[k], t, P);
        int ar = 0, ai = 0;
        for (int j = j0; j < T; j += U, --t) {
            int mr, mi;
            mix(wide_at<F>(a.in, a.hist, M, HT, t, s), tab[p], mr, mi);
            const int h = (int) a.taps[j];
            ar += h * mr;
            ai += h * mi;
            p = (p == 0) ? P - 1 : p - 1;
        }
        a.out[(size_t) m * M * a.K + (size_t) s * a.K + k] = pack2(sat16((ar + 16384) >> 15), sat16((ai + 16384) >> 15));
    }
}

// the new carry, as converted words whatever the format: hist_out[i] = the call's wide sample len - H + i, from the input
// or (calls shorter than the carry) the old carry
template <int F>
__global__ __launch_bounds__(256) void channeliser_carry_kernel(const void *__restrict__ in, const uint32_t *__restrict__ hist_in,
                                                         uint32_t *__restrict__ hist_out, int M, int H, int len)
{
    const long long idx = (long long) blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long) H * M) return;
    const int i = (int) (idx / M), s = (int) (idx % M);
    const long long t = (long long) len - H + i;
    hist_out[idx] = t >= 0 ? wide_word<F>(wide_load<F>(in, (size_t) t * M + s)) : hist_in[(size_t) (len + i) * M + s];
}

// ---- the launches of one format's instances (declared in kernels.h); a unit instantiates those of its kernels ----

// the fast form's (K, NA) instances: NA 4, 8, 17, and 33 for K <= 2, at an integer ratio; the one bucket of 17
// (RESAMP_FAST_NA) at a rational one
template <int K, int F, bool RATIONAL>
hipError_t wide_fast_launch_k(const WideLaunch &a, dim3 grid, hipStream_t stream)
{
    switch (a.NA) {
    case 17: hipLaunchKernelGGL((channeliser_kernel<K, 17, F, RATIONAL>), grid, dim3(64), 0, stream, a); return hipSuccess;
    case 4:
        if constexpr (!RATIONAL) { hipLaunchKernelGGL((channeliser_kernel<K, 4, F, false>), grid, dim3(64), 0, stream, a); return hipSuccess; }
        break;
    case 8:
        if constexpr (!RATIONAL) { hipLaunchKernelGGL((channeliser_kernel<K, 8, F, false>), grid, dim3(64), 0, stream, a); return hipSuccess; }
        break;
    case 33:
        if constexpr (!RATIONAL && K <= 2) { hipLaunchKernelGGL((channeliser_kernel<K, 33, F, false>), grid, dim3(64), 0, stream, a); return hipSuccess; }
        break;
    }
    return hipErrorInvalidValue;
}

template <int F, bool RATIONAL>
hipError_t wide_fast_launch(const WideLaunch &a, dim3 grid, hipStream_t stream)
{
    switch (a.K) {
    case 1: return wide_fast_launch_k<1, F, RATIONAL>(a, grid, stream);
    case 2: return wide_fast_launch_k<2, F, RATIONAL>(a, grid, stream);
    case 3: return wide_fast_launch_k<3, F, RATIONAL>(a, grid, stream);
    case 4: return wide_fast_launch_k<4, F, RATIONAL>(a, grid, stream);
    default: return hipErrorInvalidValue;
    }
}

template <int F>
void wide_direct_launch(const WideLaunch &a, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL(channeliser_direct_kernel<F>, grid, dim3(64), 0, stream, a);
}

template <int F>
void wide_carry_launch(const WideLaunch &a, uint32_t *hist_out, hipStream_t stream)
{
    const long long n = (long long) a.H * a.M;
    hipLaunchKernelGGL(channeliser_carry_kernel<F>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, a.in, a.hist, hist_out,
                       a.M, a.H, a.len);
}

} // namespace gnuais
