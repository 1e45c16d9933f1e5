// iq_disc.hip -- complex baseband in: the FM discriminator that turns int16 I/Q pairs into the int16 audio the
// receive chain takes (gnuais_batch_run_iq, include/gnuais_hip.h).  Not part of the reference (it reads
// discriminator audio from a sound card); its arithmetic is defined exactly in the header so that a restatement in
// NumPy matches it bit for bit (tests/iq_ref.py).
//
// Layout: in [len][N] pairs of (I, Q) int16 = one 32-bit word per (row, channel); out [len][N] int16.  A lane owns
// CPL adjacent channels (CPL = 4, 2 or 1: the widest the channel count and the pointers' alignment allow), so that a
// wave's load of one row is 64 * 4 * CPL contiguous bytes and its store 64 * 2 * CPL.  A thread walks a segment of T
// consecutive rows and keeps the previous pair in registers; a segment starts from the row before it, the first
// segment from the carry.  The carry is read and written by the SAME thread (the one of the first segment: it stores
// the call's last row after its loop), so no launch has two threads on one carry word.
//
// fp32 throughout, every operation of the definition rounded on its own: the library builds with -ffp-contract=off
// (no product is fused into a sum), and the division is the correctly rounded one (v_div_scale / v_div_fmas /
// v_div_fixup, whose internal fused steps are part of that sequence; tests/test_iq_cpu.py looks for it in the ISA).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gnuais {
namespace {

// the fp32 constants of the definition (include/gnuais_hip.h), as bit patterns
__device__ __forceinline__ float f32_bits(uint32_t u) { return __uint_as_float(u); }

__device__ __forceinline__ int16_t disc_one(uint32_t cur, uint32_t prev)
{
    const float A1 = f32_bits(0x3f7ff738u), A3 = f32_bits(0xbea91d04u), A5 = f32_bits(0x3e3876e2u),
                A7 = f32_bits(0xbdae5a36u), A9 = f32_bits(0x3caaae5fu);
    const float PI = f32_bits(0x40490fdbu), HALF_PI = f32_bits(0x3fc90fdbu), G = f32_bits(0x4622f983u);
    const float I = (float) (int16_t) (cur & 0xffffu), Q = (float) (int16_t) (cur >> 16);
    const float Ip = (float) (int16_t) (prev & 0xffffu), Qp = (float) (int16_t) (prev >> 16);
    const float re = I * Ip + Q * Qp;            // no contraction: two products, one sum, each rounded
    const float im = Q * Ip - I * Qp;
    const float ax = fabsf(re), ay = fabsf(im);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = (mx == 0.0f) ? 0.0f : mn / mx;
    const float s = t * t;
    float p = t * (A1 + s * (A3 + s * (A5 + s * (A7 + s * A9))));
    if (ay > ax) p = HALF_PI - p;
    if (re < 0.0f) p = PI - p;                   // ordered compares: -0.0 is not < 0
    if (im < 0.0f) p = -p;
    const float o = fminf(fmaxf(rintf(p * G), -32768.0f), 32767.0f);
    return (int16_t) (int) o;
}

template <int CPL> struct Vec;
template <> struct Vec<1> { using In = uint32_t; using Out = int16_t; };
template <> struct Vec<2> { using In = uint2; using Out = uint32_t; };
template <> struct Vec<4> { using In = uint4; using Out = uint2; };

__device__ __forceinline__ void words(uint32_t v, uint32_t *w) { w[0] = v; }
__device__ __forceinline__ void words(uint2 v, uint32_t *w) { w[0] = v.x; w[1] = v.y; }
__device__ __forceinline__ void words(uint4 v, uint32_t *w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }

__device__ __forceinline__ uint32_t pack2(int16_t a, int16_t b)
{
    return (uint32_t) (uint16_t) a | ((uint32_t) (uint16_t) b << 16);
}

template <int CPL>
__device__ __forceinline__ typename Vec<CPL>::Out disc_vec(const uint32_t *cur, const uint32_t *prev)
{
    if constexpr (CPL == 1) {
        return disc_one(cur[0], prev[0]);
    } else if constexpr (CPL == 2) {
        return pack2(disc_one(cur[0], prev[0]), disc_one(cur[1], prev[1]));
    } else {
        return make_uint2(pack2(disc_one(cur[0], prev[0]), disc_one(cur[1], prev[1])),
                          pack2(disc_one(cur[2], prev[2]), disc_one(cur[3], prev[3])));
    }
}

} // namespace

// grid: 1-D, block b = (segment b / n_groups, channel block b % n_groups): consecutive workgroups sweep one band of
// rows across all channels.  256 threads; thread = CPL channels; N % CPL == 0.
template <int CPL>
__global__ __launch_bounds__(256) void iq_discriminator_kernel(const uint32_t *__restrict__ iq, int16_t *__restrict__ out,
                                                               uint32_t *__restrict__ carry, int N, int len, int T,
                                                               int n_groups)
{
    using In = typename Vec<CPL>::In;
    using Out = typename Vec<CPL>::Out;
    const int grp = (int) (blockIdx.x % (unsigned) n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) n_groups);
    const int c0 = (grp * 256 + (int) threadIdx.x) * CPL;
    if (c0 >= N) return;
    const int r0 = seg * T;
    if (r0 >= len) return;
    const int r1 = min(r0 + T, len);
    const size_t rowv = (size_t) (N / CPL);           // a row in units of In
    const In *src = reinterpret_cast<const In *>(iq) + (size_t) (c0 / CPL);
    Out *dst = reinterpret_cast<Out *>(out) + (size_t) (c0 / CPL);

    uint32_t prev[CPL], cur[CPL];
    if (seg == 0)
        words(*reinterpret_cast<const In *>(carry + c0), prev);
    else
        words(src[(size_t) (r0 - 1) * rowv], prev);
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        words(src[(size_t) r * rowv], cur);
        dst[(size_t) r * rowv] = disc_vec<CPL>(cur, prev);
#pragma unroll
        for (int j = 0; j < CPL; ++j) prev[j] = cur[j];
    }
    if (seg == 0)                                      // the carry's only reader in this launch was this thread
        *reinterpret_cast<In *>(carry + c0) = src[(size_t) (len - 1) * rowv];
}

hipError_t launch_iq_discriminator(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, hipStream_t stream)
{
    if (N <= 0 || len <= 0) return hipErrorInvalidValue;
    // the widest lane the channel count and the caller's pointers allow (the carry is the library's own: aligned)
    auto fits = [&](int cpl) {
        return N % cpl == 0 && (reinterpret_cast<uintptr_t>(iq) % (4u * cpl)) == 0 &&
               (reinterpret_cast<uintptr_t>(out) % (2u * cpl)) == 0;
    };
    const int cpl = fits(4) ? 4 : fits(2) ? 2 : 1;
    const int T = IQ_DISC_ROWS;
    const int lanes = N / cpl;
    const int n_groups = (lanes + 255) / 256;
    const long long n_seg = (len + T - 1) / T;
    const long long blocks = n_seg * n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned) blocks), block(256);
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(iq);
    uint32_t *c32 = reinterpret_cast<uint32_t *>(carry);
    if (cpl == 4)
        hipLaunchKernelGGL(iq_discriminator_kernel<4>, grid, block, 0, stream, in32, out, c32, N, len, T, n_groups);
    else if (cpl == 2)
        hipLaunchKernelGGL(iq_discriminator_kernel<2>, grid, block, 0, stream, in32, out, c32, N, len, T, n_groups);
    else
        hipLaunchKernelGGL(iq_discriminator_kernel<1>, grid, block, 0, stream, in32, out, c32, N, len, T, n_groups);
    return hipGetLastError();
}

} // namespace gnuais
