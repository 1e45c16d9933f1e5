// channeliser.hip -- wideband in: tune, low-pass and decimate int16 (I, Q) streams into the narrowband I/Q the
// discriminator takes (gnuais_batch_run_wideband, include/gnuais_hip.h).  Not part of the reference; all integer, defined
// exactly in the header and restated in NumPy (tests/chan_ref.py), so the device matches it bit for bit whatever the
// order of the sums.
//
// Layout: in [len][M] words (I lo, Q hi), out [len/D][M*K] words, receiver c = s*K + k.  A lane owns one stream and all
// K offsets: it reads each wide sample once, mixes it for every offset, and walks a segment of output rows.  The mixer
// row and the taps depend on the time index alone, which is the same in every lane of a workgroup (lanes are streams,
// the segment is the workgroup's), so they are uniform loads.  Results leave with vector stores only.
//
// Fast form (channeliser_kernel<K, NA>): transposed polyphase.  With wide sample i = g*D + r of group g, output m = g + a
// takes it with tap j = a*D + D-1-r, so each mixed sample feeds the NA = ceil(T/D) outputs g .. g+NA-1, whose int32
// accumulators live in registers; after group g, output g is complete, leaves, and the accumulators shift by one.  Two
// consecutive samples of a group go into one v_dot2c_i32_i16 per accumulator (__builtin_amdgcn_sdot2): the taps are
// pre-packed on the host as pairs (h[aD + D-1-r], h[aD + D-2-r]) = POLY[r/2][a], zero where a tap index is >= T or the
// group has an odd last sample.  A segment starts NA-1 groups early to fill its accumulators (the halo: (NA-1)*D wide
// samples, ~1 % of a 1500-row segment); samples before the call come from the carry, before that they are zero.
//
// Direct form (channeliser_direct_kernel): any K and T, one lane per (stream, offset), every tap mixes its sample again.
// Used only where the fast form's accumulators do not fit in registers (K > 4, or ceil(T/D) above the largest bucket):
// filters far longer than the default 16 D + 1 taps.
//
// The carry (the last T-1 wide samples per stream) is double-buffered: a launch reads one buffer and
// channeliser_carry_kernel writes the other, so no launch reads what it writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace gnuais {
namespace {

typedef short short2_t __attribute__((ext_vector_type(2)));

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

// the wide word of stream s at call index t: the call's input, the carry before it, zero before that
__device__ __forceinline__ uint32_t wide_at(const uint32_t *__restrict__ in, const uint32_t *__restrict__ hist, int M,
                                            int T, int t, int s)
{
    if (t >= 0) return in[(size_t) t * M + s];
    if (t >= -(T - 1)) return hist[(size_t) (T - 1 + t) * M + s];
    return 0u;
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

// grid: 1-D, block b = (segment b / n_groups, stream group b % n_groups); 64 threads (one wave), thread = one stream.
template <int K, int NA>
__global__ __launch_bounds__(64) void channeliser_kernel(ChanLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int rows = a.len / a.D;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const int D = a.D, M = a.M, T = a.T, NP = (D + 1) / 2;
    const uint32_t *__restrict__ in = a.in;
    const uint32_t *__restrict__ hist = a.hist;

    int p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = phase_at(a.ph0[k], (r0 - NA + 1) * D, a.per[k]);

    int acc_r[K][NA], acc_i[K][NA];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < NA; ++j) acc_r[k][j] = acc_i[k][j] = 0;

    const size_t N = (size_t) M * K;
    for (int g = r0 - NA + 1; g < r1; ++g) {
        const int t0 = g * D;
        for (int q = 0; q < NP; ++q) {
            const int t = t0 + 2 * q;
            const bool two = 2 * q + 1 < D;
            const uint32_t x0 = wide_at(in, hist, M, T, t, s);
            const uint32_t x1 = two ? wide_at(in, hist, M, T, t + 1, s) : 0u;
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
            const uint32_t *hp = a.poly + (size_t) q * NA;
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
    }
}

// grid: x = (segment, stream group) as above, y = offset k; thread = one stream at offset k.
__global__ __launch_bounds__(64) void channeliser_direct_kernel(ChanLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int k = (int) blockIdx.y;
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int rows = a.len / a.D;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const int D = a.D, M = a.M, T = a.T, P = a.per[k];
    const uint32_t *tab = a.mix + a.off[k];
    for (int m = r0; m < r1; ++m) {
        const int e = m * D + D - 1;
        int p = phase_at(a.ph0[k], e, P);
        int ar = 0, ai = 0;
        for (int j = 0; j < T; ++j) {
            int mr, mi;
            mix(wide_at(a.in, a.hist, M, T, e - j, s), tab[p], mr, mi);
            const int h = (int) a.taps[j];
            ar += h * mr;
            ai += h * mi;
            p = (p == 0) ? P - 1 : p - 1;
        }
        a.out[(size_t) m * M * a.K + (size_t) s * a.K + k] = pack2(sat16((ar + 16384) >> 15), sat16((ai + 16384) >> 15));
    }
}

// the new carry: hist_out[i] = the call's wide sample len-(T-1)+i, from the input or (short calls) the old carry
__global__ __launch_bounds__(256) void channeliser_carry_kernel(const uint32_t *__restrict__ in,
                                                                const uint32_t *__restrict__ hist_in,
                                                                uint32_t *__restrict__ hist_out, int M, int T, int len)
{
    const long long idx = (long long) blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long) (T - 1) * M) return;
    const int i = (int) (idx / M), s = (int) (idx % M);
    const int t = len - (T - 1) + i;
    hist_out[idx] = t >= 0 ? in[(size_t) t * M + s] : hist_in[(size_t) (len + i) * M + s];
}

int channeliser_fast_na(int K, int T, int D)
{
    const int na = (T + D - 1) / D;
    if (K < 1 || K > 4) return 0;
    for (int b : {4, 8, 17}) if (na <= b) return b;
    if (na <= 33 && K <= 2) return 33;
    return 0;
}

template <int K, int NA>
static void launch_fast(const ChanLaunch &a, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((channeliser_kernel<K, NA>), grid, dim3(64), 0, stream, a);
}

template <int K>
static hipError_t launch_k(const ChanLaunch &a, dim3 grid, hipStream_t stream)
{
    switch (a.NA) {
    case 4: launch_fast<K, 4>(a, grid, stream); break;
    case 8: launch_fast<K, 8>(a, grid, stream); break;
    case 17: launch_fast<K, 17>(a, grid, stream); break;
    case 33:
        if constexpr (K <= 2) { launch_fast<K, 33>(a, grid, stream); break; }
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
    return hipSuccess;
}

hipError_t launch_channeliser(const ChanLaunch &a0, uint32_t *hist_out, hipStream_t stream)
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
        case 1: e = launch_k<1>(a, grid, stream); break;
        case 2: e = launch_k<2>(a, grid, stream); break;
        case 3: e = launch_k<3>(a, grid, stream); break;
        case 4: e = launch_k<4>(a, grid, stream); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        hipLaunchKernelGGL(channeliser_direct_kernel, dim3((unsigned) blocks, (unsigned) a.K), dim3(64), 0, stream, a);
    }
    if (e != hipSuccess) return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.T > 1) {
        const long long n = (long long) (a.T - 1) * a.M;
        hipLaunchKernelGGL(channeliser_carry_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, a.in, a.hist,
                           hist_out, a.M, a.T, a.len);
    }
    return hipGetLastError();
}

} // namespace gnuais
