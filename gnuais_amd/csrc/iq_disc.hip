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
// With the AFC on (gnuais_batch_afc, afc.hip) the launch also takes that stage's block sums from the pairs while they are
// in registers (template flag AFC): a second pass over the I/Q would cost its 4 bytes a sample again.
//
// fp32 throughout, every operation of the definition rounded on its own: the library builds with -ffp-contract=off
// (no product is fused into a sum), and the division is the correctly rounded one (v_div_scale / v_div_fmas /
// v_div_fixup, whose internal fused steps are part of that sequence; tests/test_iq_cpu.py looks for it in the ISA).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iq_common.h"
#include "kernels.h"

namespace gnuais {
namespace {

// the phase formula itself is in iq_common.h (the carrier-error estimate of afc.hip takes it from ax = |re| onward)
__device__ __forceinline__ int16_t disc_one(uint32_t cur, uint32_t prev)
{
    const float I = (float) (int16_t) (cur & 0xffffu), Q = (float) (int16_t) (cur >> 16);
    const float Ip = (float) (int16_t) (prev & 0xffffu), Qp = (float) (int16_t) (prev >> 16);
    const float re = I * Ip + Q * Qp;            // no contraction: two products, one sum, each rounded
    const float im = Q * Ip - I * Qp;
    return iq_phase(re, im);
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

// The carrier-error estimate's block sums (afc.hip, include/gnuais_hip.h): r = I*Ip + Q*Qp and i = Q*Ip - I*Qp as exact
// integers, summed over the 64 rows of a block of n.  Every product fits int32 and so does i; r reaches 2^31 (all
// four values -32768), so the two products of r are widened before they are added.
typedef short i16x2 __attribute__((ext_vector_type(2)));

template <bool AFC> struct AfcSums { };   // without the sums: an empty argument, the kernel's text is the plain discriminator's
template <> struct AfcSums<true> {
    int64_t *blk;          // [nb][N][2] (R, I): a ring of block sums, block j in slot j % nb
    int nb;
    int slot0;             // the slot of the block that holds the call's first row
    int off;               // rows of that block that earlier calls filled (n0 % 64)
};

} // namespace

// grid: 1-D, block b = (segment b / n_groups, channel block b % n_groups): consecutive workgroups sweep one band of
// rows across all channels.  256 threads; thread = CPL channels; N % CPL == 0.  AFC: the block sums are taken from the
// pairs while they are in registers; the instantiations without them keep the ISA they had before there was an AFC.
template <int CPL, bool AFC>
__global__ __launch_bounds__(256) void iq_discriminator_kernel(const uint32_t *__restrict__ iq, int16_t *__restrict__ out,
                                                               uint32_t *__restrict__ carry, int N, int len, int T,
                                                               int n_groups, AfcSums<AFC> afc)
{
    using In = typename Vec<CPL>::In;
    using Out = typename Vec<CPL>::Out;
    const int grp = (int) (blockIdx.x % (unsigned) n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) n_groups);
    const int c0 = (grp * 256 + (int) threadIdx.x) * CPL;
    if (c0 >= N) return;
    // with the block sums a segment is a block of n: the first one holds the 64 - off rows that complete the open block
    int r0 = seg * T, r1 = r0 + T;
    if constexpr (AFC) {
        r1 -= afc.off;
        r0 = max(r0 - afc.off, 0);
    }
    if (r0 >= len) return;
    r1 = min(r1, len);
    const size_t rowv = (size_t) (N / CPL);           // a row in units of In
    const In *src = reinterpret_cast<const In *>(iq) + (size_t) (c0 / CPL);
    Out *dst = reinterpret_cast<Out *>(out) + (size_t) (c0 / CPL);

    uint32_t prev[CPL], cur[CPL];
    int64_t sr[CPL], si[CPL];
    if constexpr (AFC) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) sr[j] = si[j] = 0;
    }
    if (seg == 0)
        words(*reinterpret_cast<const In *>(carry + c0), prev);
    else
        words(src[(size_t) (r0 - 1) * rowv], prev);
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        words(src[(size_t) r * rowv], cur);
        dst[(size_t) r * rowv] = disc_vec<CPL>(cur, prev);
        if constexpr (AFC) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int I = (int16_t) (cur[j] & 0xffffu), Q = (int16_t) (cur[j] >> 16);
                const int Ip = (int16_t) (prev[j] & 0xffffu), Qp = (int16_t) (prev[j] >> 16);
                // r - 1 fits int32 where r = 2^31 does not: one v_dot2_i32_i16 (no clamp), the ones are added after the loop
                sr[j] += (int64_t) __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, cur[j]), __builtin_bit_cast(i16x2, prev[j]), -1, false);
                si[j] += (int64_t) (Q * Ip - I * Qp);
            }
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) prev[j] = cur[j];
    }
    if (seg == 0)                                      // the carry's only reader in this launch was this thread
        *reinterpret_cast<In *>(carry + c0) = src[(size_t) (len - 1) * rowv];
    if constexpr (AFC) {
        // one thread per (block, channel) in a launch: the open block is added to, a block that starts here is set
        int slot = afc.slot0 + seg;
        if (slot >= afc.nb) slot -= afc.nb;
        int64_t *p = afc.blk + ((size_t) slot * (size_t) N + (size_t) c0) * 2;
        const bool open = seg == 0 && afc.off != 0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            p[2 * j] = (open ? p[2 * j] : 0) + sr[j] + (int64_t) (r1 - r0);
            p[2 * j + 1] = (open ? p[2 * j + 1] : 0) + si[j];
        }
    }
}

template <bool AFC>
static hipError_t launch(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, int off, AfcSums<AFC> afc,
                         hipStream_t stream)
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
    const long long n_seg = (off + len + T - 1) / T;
    const long long blocks = n_seg * n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned) blocks), block(256);
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(iq);
    uint32_t *c32 = reinterpret_cast<uint32_t *>(carry);
    if (cpl == 4)
        hipLaunchKernelGGL((iq_discriminator_kernel<4, AFC>), grid, block, 0, stream, in32, out, c32, N, len, T, n_groups, afc);
    else if (cpl == 2)
        hipLaunchKernelGGL((iq_discriminator_kernel<2, AFC>), grid, block, 0, stream, in32, out, c32, N, len, T, n_groups, afc);
    else
        hipLaunchKernelGGL((iq_discriminator_kernel<1, AFC>), grid, block, 0, stream, in32, out, c32, N, len, T, n_groups, afc);
    return hipGetLastError();
}

hipError_t launch_iq_discriminator(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, hipStream_t stream)
{
    return launch<false>(iq, out, carry, N, len, 0, {}, stream);
}

hipError_t launch_iq_discriminator_afc(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, int64_t *blk,
                                       int nb, unsigned long long n0, hipStream_t stream)
{
    static_assert(IQ_DISC_ROWS == AFC_BLOCK, "a segment is a block");
    if (!blk || len / AFC_BLOCK + 2 > nb) return hipErrorInvalidValue;       // a call's blocks are distinct slots
    const AfcSums<true> afc{blk, nb, (int) (n0 / AFC_BLOCK % (unsigned) nb), (int) (n0 % AFC_BLOCK)};
    return launch<true>(iq, out, carry, N, len, afc.off, afc, stream);
}

} // namespace gnuais
