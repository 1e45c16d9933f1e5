// frame_signal.hip -- the signal power and the carrier error of every decoded frame (definition: include/gnuais_hip.h,
// gnuais_batch_frame_signal).  Two kernels, both launched only while the feature is on; no chain kernel changes.
//
// iq_power_kernel, one launch per I/Q-type call on the caller's stream, in front of the discriminator: the sums
// P = I^2 + Q^2, r = I*Ip + Q*Qp and i = Q*Ip - I*Qp over every block of 64 rows of n the call touches, into the ring
// [block mod RB][N][3] int64.  It reads the I/Q the discriminator reads.  The mapping is the discriminator's
// (iq_disc.hip): a lane owns CPL = 4, 2 or 1 adjacent channels, a thread walks the rows of one block of n and keeps the
// previous pair in registers.  The stage has a carry of its own -- the last pair of the run of I/Q-type calls -- which
// the call's first thread per channel reads and, after its loop, replaces: one thread per carry word in a launch.  That
// thread also completes the block the previous call left open: it adds to the slot, where every other thread sets
// its slot.  The first call of a run (n0 == v0) starts from the pair (0, 0) and sets: the rows of its first block that
// lie before v0 count as zero, and no valid record reads that block (64 j_lo >= v0).  No word has two writers in a launch.
//
// frame_signal_kernel, one launch per call behind the frame_time launch on K3's stream: lane = frame record,
// grid-stride.  A record with t < 0 gets (0, 0, 0); a record with n0 <= t < n0 + len is this call's and gets the sums of
// its span (frame_signal.h); every other record is left alone.  Nothing is carried, so a launch is idempotent and the
// drains, discard_frames and the resets have nothing to clear (as frame_time.hip argues for the times).
//
// Why the stage has no entry of its own in the drain table (batch.h: gnuais_batch::last).  The ingest kernel is launched
// exactly where the discriminator is launched, on the same stream, so the discriminator's entry already drains it: the
// carry and the open block go from launch to launch in that stream's order, and a call on another stream waits for the
// recorded one first.  The frame kernel reads blocks that end at or before row q + 1 <= n0 + len: all of them were
// complete when this call's ingest launch ended, which is in front of this call's K1 and so in front of its K3.  Later
// ingest launches write blocks beyond those, in slots the ring's size keeps apart from every block a pending frame
// launch can still read (the bound is derived where the size is computed, capi_ingest.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_signal.h"
#include "iq_common.h"
#include "kernels.h"

namespace gnuais {

namespace {

typedef short i16x2 __attribute__((ext_vector_type(2)));

// a lane's load of one row as a native vector (an operand of the asm statement below, which HIP's uint4 cannot be)
template <int CPL> struct Nat { typedef uint32_t T __attribute__((ext_vector_type(CPL))); };
template <> struct Nat<1> { typedef uint32_t T; };
__device__ __forceinline__ void words(uint32_t __attribute__((ext_vector_type(2))) v, uint32_t *w) { w[0] = v.x; w[1] = v.y; }
__device__ __forceinline__ void words(uint32_t __attribute__((ext_vector_type(4))) v, uint32_t *w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }

constexpr int FS_THREADS = 256;
constexpr int FS_AHEAD = 8;            // rows a thread of the ingest kernel has in flight
constexpr int FS_MAX_BLOCKS = 1024;     // grid-stride beyond that: the host does not know the ring's count

} // namespace

// grid: 1-D, block b = (segment b / n_groups, channel block b % n_groups), a segment = the rows of one block of n: the
// first one holds the 64 - off rows that complete the open block.  256 threads; thread = CPL channels; N % CPL == 0.
// first: the call starts a run (n0 == v0): the previous pair is (0, 0) and the open block is set, not added to.
template <int CPL>
__global__ __launch_bounds__(FS_THREADS) void iq_power_kernel(const uint32_t *__restrict__ iq, uint32_t *__restrict__ carry,
                                                              int64_t *__restrict__ ring, int N, int len, int n_groups,
                                                              int RB, int slot0, int off, int first)
{
    using In = typename Vec<CPL>::In;
    const int grp = (int) (blockIdx.x % (unsigned) n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) n_groups);
    const int c0 = (grp * FS_THREADS + (int) threadIdx.x) * CPL;
    if (c0 >= N) return;
    const int r0 = max(seg * FS_BLOCK - off, 0);
    if (r0 >= len) return;
    const int r1 = min((seg + 1) * FS_BLOCK - off, len);
    const size_t rowv = (size_t) (N / CPL);           // a row in units of In
    const In *src = reinterpret_cast<const In *>(iq) + (size_t) (c0 / CPL);

    // The sums are taken without a 64-bit operation or an unpacked value in the loop (it is otherwise bound by its vector
    // instructions, not by its 4 bytes a sample): every term is a v_dot2_i32_i16 that accumulates in place.  A partner
    // vector p = (p0, p1) is split per half into ph = p >> 8 (signed) and pl = p & 255, so that
    //   (I, Q).p = 256 * (I, Q).ph + (I, Q).pl,   |(I, Q).ph| <= 2^23,   0 <= |(I, Q).pl| < 2^24:
    // 64 rows of either fit an int32, and the two accumulators meet in 64 bits after the loop.
    //   P = (I, Q).(I, Q);   r = (I, Q).(Ip, Qp);
    //   i = Q*Ip - I*Qp: with ~Qp = -Qp - 1 (a bit flip, where -Qp itself leaves int16 for Qp = -32768),
    //       (I, Q).(~Qp, Ip) = i - I; the block's sum of I is taken beside it as (I, Q).(1, 0).
    // The split of (~Q, I) is the split of (I, Q) with its halves swapped and the low one flipped: (~Q) >> 8 = ~(Q >> 8).
    const i16x2 one_zero = {1, 0};
    uint32_t cur[CPL], ph[CPL], pl[CPL], xh[CPL], xl[CPL];      // of the previous pair: its split, and that of (~Qp, Ip)
    int pa[CPL], pb[CPL], ra[CPL], rb[CPL], ia[CPL], ib[CPL], sI[CPL];
    if (seg != 0) {
        words(src[(size_t) (r0 - 1) * rowv], cur);
    } else if (first) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) cur[j] = 0u;
    } else {
        words(*reinterpret_cast<const In *>(carry + c0), cur);
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        pa[j] = pb[j] = ra[j] = rb[j] = ia[j] = ib[j] = sI[j] = 0;
        ph[j] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, cur[j]) >> 8);
        pl[j] = cur[j] & 0x00ff00ffu;
        xh[j] = ((ph[j] >> 16) | (ph[j] << 16)) ^ 0x0000ffffu;
        xl[j] = ((pl[j] >> 16) | (pl[j] << 16)) ^ 0x000000ffu;
    }
    using NV = typename Nat<CPL>::T;
    const NV *srcn = reinterpret_cast<const NV *>(src);
    auto row = [&](const NV &v) {
        words(v, cur);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const i16x2 a = __builtin_bit_cast(i16x2, cur[j]);
            const uint32_t h = __builtin_bit_cast(uint32_t, a >> 8), l = cur[j] & 0x00ff00ffu;
            pa[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, h), pa[j], false);
            pb[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, l), pb[j], false);
            ra[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, ph[j]), ra[j], false);
            rb[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, pl[j]), rb[j], false);
            ia[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, xh[j]), ia[j], false);
            ib[j] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(i16x2, xl[j]), ib[j], false);
            sI[j] = __builtin_amdgcn_sdot2(a, one_zero, sI[j], false);
            ph[j] = h;
            pl[j] = l;
            xh[j] = ((h >> 16) | (h << 16)) ^ 0x0000ffffu;
            xl[j] = ((l >> 16) | (l << 16)) ^ 0x000000ffu;
        }
    };
    // FS_AHEAD rows are loaded before the first of them is used: the rows of a block are 4 N bytes apart, and a thread
    // that waits for each load before it asks for the next leaves the memory pipe idle
    int r = r0;
    for (; r + FS_AHEAD <= r1; r += FS_AHEAD) {
        NV v[FS_AHEAD];
#pragma unroll
        for (int k = 0; k < FS_AHEAD; ++k) v[k] = srcn[(size_t) (r + k) * rowv];
        // all of them live at one point: the scheduler otherwise sinks each load to its use and keeps two in flight
        static_assert(FS_AHEAD == 8, "the operands below");
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
#pragma unroll
        for (int k = 0; k < FS_AHEAD; ++k) row(v[k]);
    }
    for (; r < r1; ++r) row(srcn[(size_t) r * rowv]);
    if (seg == 0)                                      // the carry's only reader in this launch was this thread
        *reinterpret_cast<In *>(carry + c0) = src[(size_t) (len - 1) * rowv];
    // one thread per (block, channel) in a launch
    const int slot = (int) ((unsigned) (slot0 + seg) % (unsigned) RB);
    int64_t *p = ring + ((size_t) slot * (size_t) N + (size_t) c0) * 3;
    const bool add = seg == 0 && off != 0 && !first;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        p[3 * j] = (add ? p[3 * j] : 0) + (int64_t) pa[j] * 256 + (int64_t) pb[j];
        p[3 * j + 1] = (add ? p[3 * j + 1] : 0) + (int64_t) ra[j] * 256 + (int64_t) rb[j];
        p[3 * j + 2] = (add ? p[3 * j + 2] : 0) + (int64_t) ia[j] * 256 + (int64_t) ib[j] + (int64_t) sI[j];
    }
}

namespace {

__global__ __launch_bounds__(FS_THREADS) void frame_signal_kernel(
    const uint32_t *__restrict__ frames, const uint32_t *__restrict__ frame_count, uint32_t frame_cap,
    const long long *__restrict__ times, const int64_t *__restrict__ ring, int RB, int N, uint2 *__restrict__ signal,
    long long n0, int len, uint32_t pllinc, int n_taps, int afc_window, long long v0)
{
    const uint32_t cnt = frame_count[0];
    const uint32_t have = cnt < frame_cap ? cnt : frame_cap;
    for (uint32_t i = blockIdx.x * FS_THREADS + threadIdx.x; i < have; i += gridDim.x * FS_THREADS) {
        const long long t = times[i];
        if (t >= 0 && (t < n0 || t >= n0 + (long long) len)) continue;      // another call's
        const uint32_t *rec = frames + (size_t) i * 16;
        const uint32_t c = rec[0];
        uint2 out = make_uint2(0u, 0u);
        long long j_lo;
        int nb;
        if (c < (uint32_t) N && fs_span(t, (int) (rec[15] >> 16), pllinc, n_taps, afc_window, v0, &j_lo, &nb)) {
            int slot = (int) (j_lo % (long long) RB);
            long long sp = 0, sr = 0, si = 0;
            for (int k = 0; k < nb; ++k) {
                const int64_t *p = ring + ((size_t) slot * (size_t) N + (size_t) c) * 3;
                sp += p[0];
                sr += p[1];
                si += p[2];
                if (++slot == RB) slot = 0;
            }
            const uint32_t power = (uint32_t) (sp / ((long long) FS_BLOCK * nb));
            const int16_t ferr = iq_phase((float) sr, (float) si);
            out = make_uint2(power, (uint32_t) (uint16_t) ferr | ((uint32_t) nb << 16));
        }
        signal[i] = out;
    }
}

} // namespace

hipError_t launch_iq_power(const int16_t *iq, uint32_t *carry, int64_t *ring, int RB, int N, int len,
                           unsigned long long n0, bool first, hipStream_t stream)
{
    // a call's blocks are distinct slots
    if (!iq || !carry || !ring || N <= 0 || len <= 0 || RB < len / FS_BLOCK + 2) return hipErrorInvalidValue;
    // the widest lane the channel count and the caller's pointer allow (carry and ring are the library's own: aligned)
    auto fits = [&](int cpl) { return N % cpl == 0 && (reinterpret_cast<uintptr_t>(iq) % (4u * cpl)) == 0; };
    const int cpl = fits(4) ? 4 : fits(2) ? 2 : 1;
    const int n_groups = (N / cpl + FS_THREADS - 1) / FS_THREADS;
    const int off = (int) (n0 % FS_BLOCK), slot0 = (int) (n0 / FS_BLOCK % (unsigned) RB);
    const long long blocks = (long long) ((off + len + FS_BLOCK - 1) / FS_BLOCK) * n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned) blocks), block(FS_THREADS);
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(iq);
    if (cpl == 4)
        hipLaunchKernelGGL(iq_power_kernel<4>, grid, block, 0, stream, in32, carry, ring, N, len, n_groups, RB, slot0, off, (int) first);
    else if (cpl == 2)
        hipLaunchKernelGGL(iq_power_kernel<2>, grid, block, 0, stream, in32, carry, ring, N, len, n_groups, RB, slot0, off, (int) first);
    else
        hipLaunchKernelGGL(iq_power_kernel<1>, grid, block, 0, stream, in32, carry, ring, N, len, n_groups, RB, slot0, off, (int) first);
    return hipGetLastError();
}

hipError_t launch_frame_signal(const FrameSignalLaunch &a, hipStream_t stream)
{
    if (!a.frames || !a.frame_count || !a.times || !a.ring || !a.signal || a.N <= 0 || a.RB <= 0 || a.pllinc == 0 ||
        a.n0 < 0)
        return hipErrorInvalidValue;
    const unsigned want = (a.frame_cap + FS_THREADS - 1) / FS_THREADS;
    const unsigned blocks = want < 1u ? 1u : want > (unsigned) FS_MAX_BLOCKS ? (unsigned) FS_MAX_BLOCKS : want;
    hipLaunchKernelGGL(frame_signal_kernel, dim3(blocks), dim3(FS_THREADS), 0, stream, (const uint32_t *) a.frames,
                       a.frame_count, a.frame_cap, (const long long *) a.times, a.ring, a.RB, a.N, (uint2 *) a.signal,
                       (long long) a.n0, a.len, a.pllinc, a.n_taps, a.afc_window, (long long) a.v0);
    return hipGetLastError();
}

} // namespace gnuais
