// frame_time.hip -- the receive time of every decoded frame, in chain rows (definition: include/gnuais_hip.h,
// gnuais_batch_frame_times).
//
// One launch per call, behind K3 on K3's stream, only while the feature is on.  Everything it needs is on the device
// after K3: the frame ring, the deframer's carried bit count ctl[2] / ctl[5] (bits fed since reset, AFTER this call) and
// the PLL stage's per-segment bit counts segcnt[N][n_seg] of the call's hand-off set.  No chain kernel changes.
//
// Which records are this call's: those whose 37-bit end_bit lies among the bits this call fed, i.e.
// r = (fed_after - 1 - end_bit) mod 2^37 < sum of the call's segment counts.  No "timed up to" word is kept: there is
// then no state that finish_drain(), gnuais_batch_discard_frames() and the resets would have to clear with the ring's
// count, and a launch is idempotent.  The price is that records earlier calls left undrained in the ring are looked at
// again (two words of the record and two of ctl each; the early-out below needs no walk).
//
// Lane = frame record.  r counts the bits of the channel BEHIND the closing bit, so the segments are walked from the
// call's last one back: the first s with r < c_s holds the bit, as its slice j = c_s - 1 - r.  At most n_seg (24 at C3,
// 94 at C5) words of one row of segcnt, L2-resident (K3's deframer read them a moment ago).  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gnuais {

namespace {

constexpr int FT_BLOCK = 256;
constexpr int FT_MAX_BLOCKS = 1024;     // grid-stride beyond that: the host does not know the ring's count

__global__ __launch_bounds__(FT_BLOCK) void frame_time_kernel(
    const uint32_t *__restrict__ frames, const uint32_t *__restrict__ frame_count, uint32_t frame_cap,
    const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ segcnt, long long *__restrict__ times,
    int N, int n_seg, int seg_cap, int len, long long n0)
{
    const uint32_t cnt = frame_count[0];
    const uint32_t have = cnt < frame_cap ? cnt : frame_cap;
    const unsigned long long M37 = (1ull << 37) - 1ull;
    // len <= 0: a gnuais_batch_decode_bits() launch -- bits without samples, every segment may hold some
    const int n_used = len > 0 ? (len + SEG_LEN - 1) / SEG_LEN : n_seg;
    const unsigned long long call_max = (unsigned long long) n_used * (unsigned long long) seg_cap;
    const size_t n_ = (size_t) N;
    for (uint32_t i = blockIdx.x * FT_BLOCK + threadIdx.x; i < have; i += gridDim.x * FT_BLOCK) {
        const uint32_t *rec = frames + (size_t) i * 16;
        const uint32_t c = rec[0];
        if (c >= (uint32_t) N) continue;
        // the record's 37-bit stamp: end_bit, and bits 5:1 of the flags byte (byte 61 = bits 15:8 of word 15)
        const unsigned long long e = (unsigned long long) rec[1] | ((unsigned long long) ((rec[15] >> 9) & 31u) << 32);
        const unsigned long long fed = (unsigned long long) ctl[2 * n_ + c] | ((unsigned long long) (ctl[5 * n_ + c] & 31u) << 32);
        unsigned long long r = (fed - 1ull - e) & M37;      // bits of the channel behind the closing bit
        if (r >= call_max) continue;                        // closed by an earlier call
        const uint32_t *__restrict__ row = segcnt + (size_t) c * (size_t) n_seg;
        for (int s = n_used - 1; s >= 0; --s) {
            uint32_t cs = row[s];
            if (cs > (uint32_t) seg_cap) cs = (uint32_t) seg_cap;       // as the deframer reads a pack
            if (r < cs) {
                long long t = -1;
                if (len > 0) {
                    const long long j = (long long) cs - 1 - (long long) r;
                    const long long ls = len - s * SEG_LEN < SEG_LEN ? len - s * SEG_LEN : SEG_LEN;
                    t = n0 + (long long) s * SEG_LEN + ((2 * j + 1) * ls) / (2 * (long long) cs);
                }
                times[i] = t;
                break;
            }
            r -= cs;
        }
    }
}

// times[order[j]] -> out[j]: the permutation of the sorted drain (nmea_device.hip: frames_sort)
__global__ __launch_bounds__(FT_BLOCK) void frame_time_gather_kernel(const long long *__restrict__ times,
                                                                     const uint32_t *__restrict__ order, int n,
                                                                     long long *__restrict__ out)
{
    const int j = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (j < n) out[j] = times[order[j]];
}

} // namespace

hipError_t launch_frame_times(const FrameTimeLaunch &a, hipStream_t stream)
{
    if (!a.frames || !a.frame_count || !a.ctl || !a.segcnt || !a.times || a.N <= 0 || a.n_seg <= 0 || a.seg_words <= 0 ||
        a.len > a.n_seg * SEG_LEN)
        return hipErrorInvalidValue;
    const unsigned want = (a.frame_cap + FT_BLOCK - 1) / FT_BLOCK;
    const unsigned blocks = want < 1u ? 1u : want > (unsigned) FT_MAX_BLOCKS ? (unsigned) FT_MAX_BLOCKS : want;
    hipLaunchKernelGGL(frame_time_kernel, dim3(blocks), dim3(FT_BLOCK), 0, stream, (const uint32_t *) a.frames,
                       a.frame_count, a.frame_cap, a.ctl, a.segcnt, (long long *) a.times, a.N, a.n_seg, a.seg_words * 32,
                       a.len, (long long) a.n0);
    return hipGetLastError();
}

hipError_t launch_frame_times_gather(const int64_t *times, const uint32_t *order, int n, int64_t *out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(frame_time_gather_kernel, dim3((n + FT_BLOCK - 1) / FT_BLOCK), dim3(FT_BLOCK), 0, stream,
                       (const long long *) times, order, n, (long long *) out);
    return hipGetLastError();
}

} // namespace gnuais
