// afc.hip -- the carrier-error stage behind the discriminator (gnuais_batch_afc, include/gnuais_hip.h): the estimate
// e_j of each block of 64 rows from the window sums of r and i, and the corrected audio out[n] = a[n - L] - e.  The
// block sums themselves are taken by the discriminator while the pairs are in its registers (iq_disc.hip,
// iq_discriminator_afc_kernel).  Everything but the phase of a window sum is integer, so no order matters; the phase
// is the discriminator's own function (iq_common.h) entered with the two sums converted to fp32.
//
// As in iq_disc.hip no word that lives from call to call is touched by two threads of one launch: a block sum is
// written by the discriminator's thread of that (block, channel) and only read here; slot n % L of the delay line is
// touched by the apply thread of a call's row r < L alone, which reads a[n - L] from it and then writes the slot's
// next content, the audio of the call's last row that shares the slot (its own row when the call is shorter than L).
// Rows from L on read a[n - L] from the call's own audio.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iq_common.h"
#include "kernels.h"

namespace gnuais {

constexpr int AFC_EST_CHUNK = 64;    // estimates per thread: the first window summed, the others slid (+ one block, - one)

// grid (channel groups of 256, chunks of AFC_EST_CHUNK blocks); lane = channel, so a wave's load of one block is
// 64 * 16 contiguous bytes.  Block k < 0 counts as zero; every other block of a window is complete (header).
__global__ __launch_bounds__(256) void afc_estimate_kernel(const int64_t *__restrict__ blk, int nb, int N,
                                                           int16_t *__restrict__ est, long long j_lo, int n_est, int half)
{
    const int c = (int) (blockIdx.x * 256 + threadIdx.x);
    if (c >= N) return;
    const int q0 = (int) blockIdx.y * AFC_EST_CHUNK;
    const int q1 = min(q0 + AFC_EST_CHUNK, n_est);
    const longlong2 *b2 = reinterpret_cast<const longlong2 *>(blk) + c;
    long long lo = j_lo + q0 - half, hi = j_lo + q0 + half;    // the window [lo, hi) of the chunk's first block
    int s_lo = (int) ((lo < 0 ? 0 : lo) % nb), s_hi = s_lo;    // slots of max(lo, 0) and of the next block to add
    long long sr = 0, si = 0;
    for (long long k = lo < 0 ? 0 : lo; k < hi; ++k) {
        const longlong2 v = b2[(size_t) s_hi * (size_t) N];
        sr += v.x;
        si += v.y;
        if (++s_hi == nb) s_hi = 0;
    }
    for (int q = q0;; ) {
        est[(size_t) q * (size_t) N + c] = iq_phase((float) sr, (float) si);
        if (++q >= q1) break;
        const longlong2 a = b2[(size_t) s_hi * (size_t) N];
        sr += a.x;
        si += a.y;
        if (++s_hi == nb) s_hi = 0;
        if (lo >= 0) {
            const longlong2 d = b2[(size_t) s_lo * (size_t) N];
            sr -= d.x;
            si -= d.y;
            if (++s_lo == nb) s_lo = 0;
        }
        ++lo;
    }
}

namespace {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// a - e on every int16 of a lane's vector, two's-complement wrap
__device__ __forceinline__ uint32_t sub2(uint32_t a, uint32_t e)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, e));
}
__device__ __forceinline__ int16_t sub_vec(int16_t a, int16_t e) { return (int16_t) ((uint16_t) a - (uint16_t) e); }
__device__ __forceinline__ uint32_t sub_vec(uint32_t a, uint32_t e) { return sub2(a, e); }
__device__ __forceinline__ uint2 sub_vec(uint2 a, uint2 e) { return make_uint2(sub2(a.x, e.x), sub2(a.y, e.y)); }

__device__ __forceinline__ void zero_vec(int16_t &v) { v = 0; }
__device__ __forceinline__ void zero_vec(uint32_t &v) { v = 0; }
__device__ __forceinline__ void zero_vec(uint2 &v) { v = make_uint2(0, 0); }

} // namespace

// grid as the discriminator's: block b = (segment b / n_groups, channel block b % n_groups), a segment = the rows of
// one block of n, so that one estimate serves it (L is a multiple of 64: m = n - L lies in block (n div 64) - L / 64).
// e_shift: est row of the call's first segment (negative while m < 0: those rows are 0).  d0 = n0 % L.
template <int CPL>
__global__ __launch_bounds__(256) void afc_apply_kernel(const int16_t *__restrict__ audio, int16_t *delay,
                                                        const int16_t *__restrict__ est, int16_t *__restrict__ out, int N,
                                                        int len, int L, int off, int d0, int e_shift, int n_groups)
{
    using V = typename Vec<CPL>::Out;
    const int grp = (int) (blockIdx.x % (unsigned) n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) n_groups);
    const int c0 = (grp * 256 + (int) threadIdx.x) * CPL;
    if (c0 >= N) return;
    const int r0 = max(seg * AFC_BLOCK - off, 0);
    if (r0 >= len) return;
    const int r1 = min((seg + 1) * AFC_BLOCK - off, len);
    const size_t rowv = (size_t) (N / CPL);
    const V *src = reinterpret_cast<const V *>(audio) + (size_t) (c0 / CPL);
    V *dl = reinterpret_cast<V *>(delay) + (size_t) (c0 / CPL);
    V *dst = reinterpret_cast<V *>(out) + (size_t) (c0 / CPL);
    const int e_row = seg + e_shift;
    V e;
    zero_vec(e);
    if (e_row >= 0) e = reinterpret_cast<const V *>(est)[(size_t) e_row * rowv + (size_t) (c0 / CPL)];
    const bool live = e_row >= 0;                    // else m < 0 in the whole segment: zeros
    // the call's first L rows take a[m] from the delay line and leave the slot's next content there
    int r = r0;
    int slot = (d0 + r0) % L;
    for (const int rd = min(r1, L); r < rd; ++r) {
        const V a = dl[(size_t) slot * rowv];        // a[m] of an earlier call (zero before the stream began)
        // the call's last row that shares the slot (r + kL < len, k as large as it gets)
        dl[(size_t) slot * rowv] = src[(size_t) (r + (len - 1 - r) / L * L) * rowv];
        V o;
        zero_vec(o);
        if (live) o = sub_vec(a, e);
        dst[(size_t) r * rowv] = o;
        if (++slot == L) slot = 0;
    }
    // the others take it from the call's own audio: loads and stores of two buffers that do not overlap
#pragma unroll 8
    for (; r < r1; ++r) {
        V o;
        zero_vec(o);
        if (live) o = sub_vec(src[(size_t) (r - L) * rowv], e);
        dst[(size_t) r * rowv] = o;
    }
}

hipError_t launch_afc_estimate(const int64_t *blk, int nb, int N, int16_t *est, long long j_lo, int n_est, int W,
                               hipStream_t stream)
{
    if (!blk || !est || N <= 0 || n_est <= 0 || j_lo < 0 || W < AFC_MIN_WINDOW || W / AFC_BLOCK + n_est > nb)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned) ((N + 255) / 256), (unsigned) ((n_est + AFC_EST_CHUNK - 1) / AFC_EST_CHUNK)), block(256);
    hipLaunchKernelGGL(afc_estimate_kernel, grid, block, 0, stream, blk, nb, N, est, j_lo, n_est, W / AFC_BLOCK / 2);
    return hipGetLastError();
}

hipError_t launch_afc_apply(const int16_t *audio, int16_t *delay, const int16_t *est, long long j_lo, int16_t *out, int N,
                            int len, int W, unsigned long long n0, hipStream_t stream)
{
    if (!audio || !delay || !est || !out || N <= 0 || len <= 0) return hipErrorInvalidValue;
    const int L = W / 2;
    // audio, delay and est are the library's own (aligned); the output may be a caller's view
    auto fits = [&](int cpl) { return N % cpl == 0 && (reinterpret_cast<uintptr_t>(out) % (2u * cpl)) == 0 &&
                                      (reinterpret_cast<uintptr_t>(audio) % (2u * cpl)) == 0; };
    const int cpl = fits(4) ? 4 : fits(2) ? 2 : 1;
    const int n_groups = (N / cpl + 255) / 256;
    const int off = (int) (n0 % AFC_BLOCK), d0 = (int) (n0 % (unsigned) L);
    // the block of row m = n - L of the call's first segment, as a row of est (row 0 = block j_lo)
    const int e_shift = (int) ((long long) (n0 / AFC_BLOCK) - L / AFC_BLOCK - j_lo);
    const long long blocks = (long long) ((off + len + AFC_BLOCK - 1) / AFC_BLOCK) * n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned) blocks), block(256);
    if (cpl == 4)
        hipLaunchKernelGGL(afc_apply_kernel<4>, grid, block, 0, stream, audio, delay, est, out, N, len, L, off, d0, e_shift, n_groups);
    else if (cpl == 2)
        hipLaunchKernelGGL(afc_apply_kernel<2>, grid, block, 0, stream, audio, delay, est, out, N, len, L, off, d0, e_shift, n_groups);
    else
        hipLaunchKernelGGL(afc_apply_kernel<1>, grid, block, 0, stream, audio, delay, est, out, N, len, L, off, d0, e_shift, n_groups);
    return hipGetLastError();
}

} // namespace gnuais
