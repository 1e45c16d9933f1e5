// hdlc_long_repair.hip -- repair of the long frames that fail the CRC by one symbol error (definition:
// include/gnuais_hip.h, gnuais_batch_long_repair; the trial itself: hdlc_repair.h with LongLimits, shared with the
// host's gnuais_long_repair_candidate).
//
// One launch per call, behind D''s (hdlc_long.hip, in its form that keeps the raw bits) on D''s stream, only while
// both features are on.  D' appended one record per frame it counted in `failed` to the call's candidate ring; how many
// is known on the device only, so the grid is fixed: workgroups of ONE wave, workgroup b takes the candidates b,
// b + blocks, ...  A call without failed long frames -- nearly every call -- costs each wave one load and an exit.
//   wave  = candidate: its record (header and 40 raw words) goes into the workgroup's LDS row, the byte-wise CRC table is
//           built once per workgroup, and only by a workgroup that has a candidate;
//   lane  = trial p, 64 per round, rawlen - 1 <= 1235 trials: 20 rounds at most.  Every trial goes through
//           trial_shape() (a popcount per word: most trials of a frame whose length is no multiple of 8 end there) and,
//           when it is well formed, the full unstuff + CRC.  A ballot and a popcount count the passing trials;
//   with exactly one, the lane that passed builds the 152-byte record in LDS, takes a slot of the long ring through the
//           ring's own counter, stores it and bumps repaired[channel].  A full ring is reported as D' reports it.
// Uniqueness does not depend on the order of the trials, so neither does the result.  The records land behind D''s in
// whatever order the waves finish; the drain sorts by (channel, 37-bit stamp).
// No scratch: every array is in LDS (row, record, table: under 1 KB).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gnuais_hip.h"
#include "hdlc_repair.h"
#include "kernels.h"

namespace gnuais {

namespace {

using LL = repair::LongLimits;
static_assert(LL::RAW_WORDS == LONG_REC_WORDS, "D''s open record");
static_assert(LL::MAX_STORED + 1 == LONG_LIMIT_BITS && LL::MIN_BITS == LONG_SHORT_BITS + 1, "D''s numbers");
static_assert(LL::MAX_CRC_BYTES == GNUAIS_LONG_MAX_BITS / 8 + 2, "the CRC of the longest frame");

__global__ __launch_bounds__(64) void hdlc_long_repair_kernel(
    const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cand_count, uint32_t cand_cap,
    int32_t *__restrict__ repaired, uint32_t *__restrict__ frames, uint32_t *__restrict__ frame_count, uint32_t frame_cap,
    int N, int blocks)
{
    __shared__ uint16_t tab[256];
    __shared__ uint32_t row[LONG_CAND_WORDS];
    __shared__ uint32_t rec[LONG_FRAME_WORDS];
    const int lane = threadIdx.x;
    uint32_t total = cand_count[0];             // final: D' ran in front of this launch
    if (total > cand_cap) total = cand_cap;
    if ((uint32_t) blockIdx.x >= total) return; // the same for the whole workgroup
    for (int q = lane; q < 256; q += 64) tab[q] = repair::crc_table_entry((uint32_t) q);

    for (uint32_t i = blockIdx.x; i < total; i += (uint32_t) blocks) {
        __syncthreads();                        // the table; the previous candidate's row and record are done with
        if (lane < LONG_CAND_WORDS) row[lane] = cand[(size_t) i * LONG_CAND_WORDS + lane];
        __syncthreads();
        const uint32_t *raw = row + LONG_CAND_HDR;
        const uint32_t c = row[0];
        int rawlen = (int) row[5];
        if (rawlen > LL::RAW_BITS) rawlen = LL::RAW_BITS;
        if (c >= (uint32_t) N) continue;        // not a record of this batch's D'
        int passing = 0, my_p = -1, my_n = 0;
        for (int p0 = 0; p0 <= rawlen - 2; p0 += 64) {
            const int p = p0 + lane;
            int n1 = 0;
            const bool ok = p <= rawlen - 2 && repair::trial_passes<LL>(raw, rawlen, p, tab, &n1);
            if (ok) { my_p = p; my_n = n1; }
            passing += __popcll(__ballot(ok));
        }
        if (passing == 1 && my_p >= 0) {        // the one lane that passed, alone
            for (int q = 0; q < LONG_FRAME_WORDS; ++q) rec[q] = 0;
            const int nbytes = my_n >> 3;       // <= 126
            (void) repair::trial_crc<LL>(raw, rawlen, my_p, nbytes + 2, tab, reinterpret_cast<uint8_t *>(rec + 5), nbytes);
            rec[0] = c;
            rec[1] = row[1];
            rec[2] = row[2];
            rec[3] = row[3];
            // flags: bit 0 CRC ok, bits 5:1 = bits 36:32 of the stamp (from the candidate), bit 6 repaired
            rec[4] = (uint32_t) my_n | ((1u | (((row[4] >> 16) & 31u) << 1) | (uint32_t) GNUAIS_FRAME_REPAIRED) << 16);
            atomicAdd(&repaired[c], 1);
            const uint32_t slot = atomicAdd(&frame_count[0], 1u);
            if (slot < frame_cap) {
                uint32_t *dst = frames + (size_t) slot * LONG_FRAME_WORDS;
                for (int q = 0; q < LONG_FRAME_WORDS; ++q) dst[q] = rec[q];
            } else {
                frame_count[1] = 1;             // ring full: frame dropped, still counted
            }
        }
    }
}

} // namespace

hipError_t launch_hdlc_long_repair(const LongRepairLaunch &a, hipStream_t stream)
{
    if (!a.cand || !a.cand_count || !a.repaired || !a.frames || !a.frame_count || a.N <= 0 || a.blocks <= 0 || a.cand_cap == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hdlc_long_repair_kernel, dim3((unsigned) a.blocks), dim3(64), 0, stream, a.cand, a.cand_count,
                       a.cand_cap, a.repaired, (uint32_t *) a.frames, a.frame_count, a.frame_cap, a.N, a.blocks);
    return hipGetLastError();
}

} // namespace gnuais
