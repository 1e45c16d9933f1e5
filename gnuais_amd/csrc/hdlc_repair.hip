// hdlc_repair.hip -- repair of the frames that fail the CRC by one symbol error (definition: include/gnuais_hip.h,
// gnuais_batch_repair; the trial itself: hdlc_repair.h, shared with the host's gnuais_repair_candidate).
//
// One launch per call, behind K3 on K3's stream and in front of the frame_time launch, only while the feature is on.
// It reads what K3 read -- cand, cand_first, cand_count of the call's hand-off set -- and K3 leaves no mark on a
// record, so it finds the failed candidates itself.  No chain kernel changes.
//
// A block of 256 threads owns K3_CH adjacent channels and enumerates their candidates as K3 does, 256 per pass.
//   Phase one: thread = candidate.  The raw record goes into the thread's row of LDS, K3's unstuff + CRC runs over
//              it; the rows that fail are listed.
//   Phase two: wave = failed candidate (taken from the list in turn), lane = trial p, stride 64.  Every trial goes
//              through trial_shape() (a popcount per word: most trials of a frame whose length is no multiple of 8 end
//              there) and, when it is well formed, the full unstuff + CRC.  A ballot and a popcount count the passing
//              trials over the strides; with exactly one, the lane that passed builds the 64-byte record in the wave's
//              LDS words, takes a slot of the frame ring through the ring's own counter and stores it.
// Uniqueness does not depend on the order of the trials, so neither does the result.  The records a call appends land
// behind K3's in whatever order the waves finish; the drains sort by (channel, 37-bit stamp).
// LDS: 256 rows of 21 words (18 raw, header, end_bit, channel), dynamic (see K3 on static shared memory and the
// register request), the byte table, the list.  No scratch: the only arrays are in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gnuais_hip.h"
#include "hdlc_repair.h"
#include "kernels.h"

namespace gnuais {

namespace {

constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / 64;
constexpr int RP_ROW = repair::RAW_WORDS + 3;       // odd: a wave's rows spread over the banks
constexpr uint32_t RP_CAND_VALID = 0x10000u;        // hdlc_crc.hip: CAND_VALID
static_assert(repair::RAW_WORDS == CAND_WORDS - CAND_HDR, "a candidate record's raw words");

__global__ __launch_bounds__(RP_BLOCK) void hdlc_repair_kernel(
    const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cand_first,
    const uint32_t *__restrict__ cand_count, int32_t *__restrict__ repaired, uint32_t *__restrict__ frames,
    uint32_t *__restrict__ flags, uint32_t frame_cap, int N, int K)
{
    __shared__ uint16_t tab[256];
    __shared__ uint32_t pre[K3_CH + 1];
    __shared__ uint16_t fail_row[RP_BLOCK];
    __shared__ uint32_t n_fail;
    __shared__ uint32_t recbuf[RP_WAVES][16];
    HIP_DYNAMIC_SHARED(uint32_t, rp_rows)           // [RP_BLOCK][RP_ROW]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c_own = blockIdx.x * K3_CH + tid;

    tab[tid] = repair::crc_table_entry((uint32_t) tid);
    if (tid < K3_CH) pre[tid + 1] = (c_own < N) ? cand_count[c_own] : 0u;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        pre[0] = 0;
        for (int q = 1; q <= K3_CH; ++q) {
            const uint32_t n = pre[q] > (uint32_t) K ? (uint32_t) K : pre[q];
            run += n;
            pre[q] = run;
        }
    }
    __syncthreads();
    const uint32_t total = pre[K3_CH];

    for (uint32_t i0 = 0; i0 < total; i0 += RP_BLOCK) {
        if (tid == 0) n_fail = 0;
        __syncthreads();
        // ---- phase one: which of this pass's candidates did K3 count in lostframes ----
        const uint32_t i = i0 + (uint32_t) tid;
        if (i < total) {
            int lo = 0, hi = K3_CH - 1;             // channel of candidate i: largest k with pre[k] <= i
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= i) lo = mid; else hi = mid - 1;
            }
            const int c = blockIdx.x * K3_CH + lo;
            const uint32_t j = i - pre[lo];
            const uint32_t slot = (cand_first[c] + j) % (uint32_t) K;
            const uint32_t *rec = cand + ((size_t) c * K + slot) * CAND_WORDS;
            const uint32_t hdr = rec[0];
            if (hdr & RP_CAND_VALID) {
                uint32_t *row = rp_rows + tid * RP_ROW;
                uint32_t raw[repair::RAW_WORDS];
#pragma unroll
                for (int q = 0; q < repair::RAW_WORDS; ++q) raw[q] = rec[CAND_HDR + q];     // one latency
#pragma unroll
                for (int q = 0; q < repair::RAW_WORDS; ++q) row[q] = raw[q];
                int rawlen = (int) ((hdr >> 17) & 0x3ffu);
                if (rawlen > repair::RAW_BITS) rawlen = repair::RAW_BITS;
                const int n = (int) (hdr & 0xffffu);
                const uint32_t crc = repair::trial_crc(row, rawlen, -1, (n >> 3) + 2, tab, nullptr, 0);
                if (crc != repair::CRC_GOOD) {
                    row[repair::RAW_WORDS] = hdr;
                    row[repair::RAW_WORDS + 1] = rec[1];
                    row[repair::RAW_WORDS + 2] = (uint32_t) c;
                    fail_row[atomicAdd(&n_fail, 1u)] = (uint16_t) tid;
                }
            }
        }
        __syncthreads();
        // ---- phase two: a wave per failed candidate, a lane per trial ----
        const uint32_t nf = n_fail;
        for (uint32_t f = (uint32_t) wave; f < nf; f += RP_WAVES) {
            const uint32_t *row = rp_rows + (int) fail_row[f] * RP_ROW;
            const uint32_t hdr = row[repair::RAW_WORDS];
            int rawlen = (int) ((hdr >> 17) & 0x3ffu);
            if (rawlen > repair::RAW_BITS) rawlen = repair::RAW_BITS;
            int passing = 0, my_p = -1, my_n = 0;
            for (int p0 = 0; p0 <= rawlen - 2; p0 += 64) {
                const int p = p0 + lane;
                int n1 = 0;
                const bool ok = p <= rawlen - 2 && repair::trial_passes(row, rawlen, p, tab, &n1);
                if (ok) { my_p = p; my_n = n1; }
                passing += __popcll(__ballot(ok));
            }
            if (passing == 1 && my_p >= 0) {        // the one lane that passed, alone
                uint32_t *out = recbuf[wave];
#pragma unroll
                for (int q = 0; q < 16; ++q) out[q] = 0;
                const int nbytes = my_n >> 3;       // <= 53
                (void) repair::trial_crc(row, rawlen, my_p, nbytes + 2, tab, reinterpret_cast<uint8_t *>(out) + 8, nbytes);
                const uint32_t c = row[repair::RAW_WORDS + 2];
                out[0] = c;
                out[1] = row[repair::RAW_WORDS + 1];
                // flags: bit 0 CRC ok, bits 5:1 = bits 36:32 of end_bit (from the candidate), bit 6 repaired
                out[15] = (out[15] & 0xffu) | ((1u | ((hdr >> 27) << 1) | (uint32_t) GNUAIS_FRAME_REPAIRED) << 8) |
                          ((uint32_t) my_n << 16);
                atomicAdd(&repaired[c], 1);
                const uint32_t idx = atomicAdd(&flags[0], 1u);
                if (idx < frame_cap) {
                    uint4 *dst = reinterpret_cast<uint4 *>(frames + (size_t) idx * 16);
                    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
                    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
                    dst[2] = make_uint4(out[8], out[9], out[10], out[11]);
                    dst[3] = make_uint4(out[12], out[13], out[14], out[15]);
                } else {
                    flags[1] = 1;                   // ring full: frame dropped, still counted
                }
            }
        }
        __syncthreads();
    }
}

} // namespace

hipError_t launch_hdlc_repair(const RepairLaunch &a, hipStream_t stream)
{
    if (!a.cand || !a.cand_first || !a.cand_count || !a.repaired || !a.frames || !a.frame_count || a.N <= 0 || a.K <= 0)
        return hipErrorInvalidValue;
    constexpr size_t RP_DYN_LDS = (size_t) RP_BLOCK * RP_ROW * sizeof(uint32_t);
    hipLaunchKernelGGL(hdlc_repair_kernel, dim3((unsigned) k3_blocks(a.N)), dim3(RP_BLOCK), RP_DYN_LDS, stream, a.cand,
                       a.cand_first, a.cand_count, a.repaired, (uint32_t *) a.frames, a.frame_count, a.frame_cap, a.N,
                       a.K);
    return hipGetLastError();
}

} // namespace gnuais
