// long_signal.hip -- the signal power and the carrier error of every long frame, and its share in the channel load
// (definition: include/gnuais_hip.h, gnuais_batch_long_frame_signal).  One kernel, launched only while the feature is on;
// no other kernel changes.
//
// long_signal_kernel, one launch per call behind D' and the long repair on K3's stream: wave = record of the long ring,
// grid-stride over waves.  A record with t < 0 gets (0, 0, 0); a record with n0 <= t < n0 + len is this call's and gets
// the sums of its span (frame_signal.h, the text frame_signal_kernel runs); every other record is left alone.  Nothing is
// carried, so a launch is idempotent and the drains and the resets have nothing to clear.
//
// Why a wave per record where frame_signal_kernel takes a lane.  A long frame's span is up to 81 blocks at 48 kHz and
// about 323 at the 192 kHz table, 24 N bytes apart in the ring, and a call closes a handful of such frames: one lane
// would walk that many dependent loads.  Here lane k takes the blocks j_lo + k, j_lo + k + 64, ...: every load of a round
// is in flight at once, and the three int64 sums meet by cross-lane adds (exact integers: the order is free).  Lane 0
// computes power and ferr and stores the record's 8 bytes.  No LDS, no atomics.
//
// The cover bytes (gnuais_batch_occupancy, with LAG of the long span): the same launch, for this call's records only,
// lanes over the blocks of the cover span (occupancy.h), same-value byte stores under the three guards of
// occ_cover_kernel: blocks in front of b0 belong to no epoch, a span that begins before the run covers nothing, and a
// span of CB blocks or more is left out (the host sized the ring beyond the longest).
//
// The ring's blocks this launch reads end at or before row q + 1 <= n0 + len and were complete when this call's ingest
// launch ended; the ring is sized for the long span while the feature is on (capi_ingest.hip), so no later ingest launch
// writes a slot a pending launch of this kernel can still read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_signal.h"
#include "iq_common.h"
#include "kernels.h"
#include "occupancy.h"

namespace gnuais {

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_LANES = 64;
constexpr int LS_WAVES = LS_THREADS / LS_LANES;
// Grid-stride beyond that: the host does not know the ring's count, only its capacity.  2048 workgroups are eight waves on
// every SIMD of the device; on a ring that holds a handful of records nearly all of them read the count and end.
// Measured at C3 with every channel closing five long frames a call (88 021 records a call, three calls in the ring):
// 64 workgroups -- one wave per compute unit walking a thousand records, each a chain of dependent loads -- added 1.14 ms
// per call.
constexpr int LS_MAX_BLOCKS = 2048;

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = LS_LANES / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, LS_LANES);
    return v;
}

__global__ __launch_bounds__(LS_THREADS) void long_signal_kernel(
    const uint32_t *__restrict__ frames, const uint32_t *__restrict__ frame_count, uint32_t frame_cap,
    const int64_t *__restrict__ ring, int RB, int N, uint2 *__restrict__ signal, long long n0, int len, uint32_t pllinc,
    int n_taps, int afc_window, long long v0, uint8_t *__restrict__ cover, int CB, long long occ_v0, long long b0)
{
    const uint32_t cnt = frame_count[0];
    const uint32_t have = cnt < frame_cap ? cnt : frame_cap;
    const int lane = (int) threadIdx.x & (LS_LANES - 1);
    const uint32_t wave = blockIdx.x * LS_WAVES + threadIdx.x / LS_LANES, n_waves = gridDim.x * LS_WAVES;
    for (uint32_t i = wave; i < have; i += n_waves) {
        const uint32_t *rec = frames + (size_t) i * LONG_FRAME_WORDS;
        const long long t = (long long) ((uint64_t) rec[2] | (uint64_t) rec[3] << 32);
        if (t >= 0 && (t < n0 || t >= n0 + (long long) len)) continue;      // another call's
        const uint32_t c = rec[0];
        const int nbits = (int) (rec[4] & 0xffffu);
        long long j_lo;
        int nb;
        const bool measured = c < (uint32_t) N && fs_span(t, nbits, pllinc, n_taps, afc_window, v0, &j_lo, &nb);
        long long sp = 0, sr = 0, si = 0;
        if (measured) {
            for (int k = lane; k < nb; k += LS_LANES) {
                const int slot = (int) ((j_lo + k) % (long long) RB);
                const int64_t *p = ring + ((size_t) slot * (size_t) N + (size_t) c) * 3;
                sp += p[0];
                sr += p[1];
                si += p[2];
            }
        }
        sp = wave_sum(sp);
        sr = wave_sum(sr);
        si = wave_sum(si);
        if (lane == 0) {
            uint2 out = make_uint2(0u, 0u);
            if (measured) {
                const uint32_t power = (uint32_t) (sp / ((long long) FS_BLOCK * nb));
                const int16_t ferr = iq_phase((float) sr, (float) si);
                out = make_uint2(power, (uint32_t) (uint16_t) ferr | ((uint32_t) nb << 16));
            }
            signal[i] = out;
        }
        if (!cover || t < 0 || c >= (uint32_t) N ||
            !occ_cover_span(t, nbits, pllinc, n_taps, afc_window, occ_v0, &j_lo, &nb))
            continue;
        const long long end = j_lo + nb;
        if (end - j_lo >= CB) continue;                          // the host sized the ring beyond the longest span
        for (long long j = (j_lo < b0 ? b0 : j_lo) + lane; j < end; j += LS_LANES)
            cover[(size_t) (j % (long long) CB) * (size_t) N + (size_t) c] = 1;
    }
}

} // namespace

hipError_t launch_long_signal(const LongSignalLaunch &a, hipStream_t stream)
{
    if (!a.frames || !a.frame_count || !a.ring || !a.signal || a.N <= 0 || a.RB <= 0 || a.pllinc == 0 || a.n0 < 0 ||
        (a.cover && (a.CB <= 0 || a.len <= 0 || a.occ_v0 < 0 || a.b0 < 0)))
        return hipErrorInvalidValue;
    const unsigned want = (a.frame_cap + LS_WAVES - 1) / LS_WAVES;
    const unsigned blocks = want < 1u ? 1u : want > (unsigned) LS_MAX_BLOCKS ? (unsigned) LS_MAX_BLOCKS : want;
    hipLaunchKernelGGL(long_signal_kernel, dim3(blocks), dim3(LS_THREADS), 0, stream, (const uint32_t *) a.frames,
                       a.frame_count, a.frame_cap, a.ring, a.RB, a.N, (uint2 *) a.signal, (long long) a.n0, a.len, a.pllinc,
                       a.n_taps, a.afc_window, (long long) a.v0, a.cover, a.CB, (long long) a.occ_v0, (long long) a.b0);
    return hipGetLastError();
}

} // namespace gnuais
