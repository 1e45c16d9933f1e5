// resampler.hip -- wideband in at a rational ratio: tune, low-pass and resample by U/D (gnuais_batch_resampler,
// include/gnuais_hip.h), for captures whose rate is no integer multiple of the chain's.  All integer, defined exactly in
// the header and restated in NumPy (tests/resample_ref.py), so the device matches it bit for bit whatever the order of
// the sums.  The integer channeliser (channeliser.hip) is the case U = 1 and keeps its own kernels; what a lane loads,
// how a format becomes a word and the mixer are its channeliser_body.h.
//
// Layout as there: in [len][M] pairs, out [len*U/D][M*K] words, receiver c = s*K + k; a lane owns one stream and all K
// offsets; the time index, and with it the mixer row, the group and its taps, is uniform over the workgroup.
//
// Fast form (resampler_kernel<K, NA, F>): transposed polyphase over GROUPS (resample_plan.h).  Group g holds the wide
// samples n with g*D <= n*U < (g+1)*D -- floor(D/U) or ceil(D/U) of them -- and each feeds rows g .. g+NA-1, whose
// int32 accumulators live in registers; after group g, row g is complete, leaves, and the accumulators shift by one.  A
// call starts on a period boundary (len is a multiple of D, so its rows are a multiple of U): call-local row g = c*U + i
// has its first sample at c*D + first[i], and its size and its tap pairs depend on i alone, so the loop carries (c, i)
// and needs no division.  Two consecutive samples of a group go into one v_dot2c_i32_i16 per accumulator; the host packed
// the taps as pairs per (i, pair, accumulator).  A segment starts NA-1 groups early (the halo); samples before the call
// come from the carry, before that they are zero.
//
// Direct form (resampler_direct_kernel<F>): any K and T, one lane per (stream, offset): row m walks the taps
// j = u_m mod U, + U, ... and mixes each sample again.  For K > 4 and prototypes longer than NA * D.
//
// The carry (the last H = ceil((T-1)/U) wide samples per stream, converted) is double-buffered as the channeliser's.
#include "channeliser_body.h"
#include "resample_plan.h"

namespace gnuais {

// grid: 1-D, block b = (segment b / n_groups, stream group b % n_groups); 64 threads (one wave), thread = one stream.
template <int K, int NA, int F>
__global__ __launch_bounds__(64) void resampler_kernel(ResampLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int U = a.U, D = a.D, M = a.M, HT = a.H + 1;
    const int rows = a.len / D * U;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const void *__restrict__ in = a.in;
    const uint32_t *__restrict__ hist = a.hist;
    const int32_t *__restrict__ groups = a.groups;
    const uint32_t *__restrict__ pairs = a.pairs;

    // the first group of the segment's halo as (period c, phase i), floor division
    const int g0 = r0 - NA + 1;
    int c = g0 / U, i = g0 % U;
    if (i < 0) { i += U; --c; }

    int p[K];
    {
        const int t_first = c * D + groups[3 * i];
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
        const int t0 = c * D + groups[3 * i], size = groups[3 * i + 1];
        const uint32_t *hg = pairs + (size_t) groups[3 * i + 2] * NA;
        const int NP = (size + 1) / 2;
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
            const uint32_t *hp = hg + (size_t) q * NA;
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
        if (++i == U) { i = 0; ++c; }
    }
}

// the direct form.  grid: x = (segment, stream group) as above, y = offset k; thread = one stream at offset k.
template <int F>
__global__ __launch_bounds__(64) void resampler_direct_kernel(ResampLaunch a)
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
        const int j0 = (int) (e % U);
        int t = (int) ((e - j0) / U);                       // < len
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
__global__ __launch_bounds__(256) void resampler_carry_kernel(const void *__restrict__ in, const uint32_t *__restrict__ hist_in,
                                                              uint32_t *__restrict__ hist_out, int M, int H, int len)
{
    const long long idx = (long long) blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long) H * M) return;
    const int i = (int) (idx / M), s = (int) (idx % M);
    const long long t = (long long) len - H + i;
    hist_out[idx] = t >= 0 ? wide_word<F>(wide_load<F>(in, (size_t) t * M + s)) : hist_in[(size_t) (len + i) * M + s];
}

namespace {

template <int F>
hipError_t launch_resampler_f(const ResampLaunch &a0, uint32_t *hist_out, hipStream_t stream)
{
    ResampLaunch a = a0;
    if (a.M <= 0 || a.K <= 0 || a.K > CHAN_MAX_K || a.U < 1 || a.D <= a.U || a.len <= 0 || a.len % a.D || a.T < 1 ||
        a.H != (a.T - 1 + a.U - 1) / a.U)
        return hipErrorInvalidValue;
    const long long rows = (long long) (a.len / a.D) * a.U;
    if (rows > 0x7fffffffLL) return hipErrorInvalidValue;
    a.n_groups = (a.M + 63) / 64;
    // segments as the channeliser's: enough waves to fill the chip, no shorter than 128 rows (the halo is NA-1 groups)
    const long long want = (rows * a.n_groups + 4095) / 4096;
    a.seg_rows = (int) std::min<long long>(2048, std::max<long long>(128, want));
    const long long n_seg = (rows + a.seg_rows - 1) / a.seg_rows;
    const long long blocks = n_seg * a.n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned) blocks);
    if (a.NA == RESAMP_FAST_NA) {
        switch (a.K) {
        case 1: hipLaunchKernelGGL((resampler_kernel<1, RESAMP_FAST_NA, F>), grid, dim3(64), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((resampler_kernel<2, RESAMP_FAST_NA, F>), grid, dim3(64), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((resampler_kernel<3, RESAMP_FAST_NA, F>), grid, dim3(64), 0, stream, a); break;
        case 4: hipLaunchKernelGGL((resampler_kernel<4, RESAMP_FAST_NA, F>), grid, dim3(64), 0, stream, a); break;
        default: return hipErrorInvalidValue;
        }
    } else if (a.NA == 0) {
        hipLaunchKernelGGL(resampler_direct_kernel<F>, dim3((unsigned) blocks, (unsigned) a.K), dim3(64), 0, stream, a);
    } else {
        return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.H > 0) {
        const long long n = (long long) a.H * a.M;
        hipLaunchKernelGGL(resampler_carry_kernel<F>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, a.in, a.hist,
                           hist_out, a.M, a.H, a.len);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_resampler(const ResampLaunch &a, int fmt, uint32_t *hist_out, hipStream_t stream)
{
    switch (fmt) {
    case FMT_CS16: return launch_resampler_f<FMT_CS16>(a, hist_out, stream);
    case FMT_CU8: return launch_resampler_f<FMT_CU8>(a, hist_out, stream);
    case FMT_CS8: return launch_resampler_f<FMT_CS8>(a, hist_out, stream);
    case FMT_CF32: return launch_resampler_f<FMT_CF32>(a, hist_out, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gnuais
