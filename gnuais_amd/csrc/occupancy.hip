// occupancy.hip -- the channel load per receiver: noise floor, busy and decoded air time per epoch of E blocks of 64 rows
// (definition: include/gnuais_hip.h, gnuais_batch_occupancy).  Three kernels, all launched only while the feature is on; no
// other kernel changes.
//
// occ_code_kernel, one launch per I/Q-type call on the caller's stream, behind iq_power_kernel and in front of the
// discriminator: lane = channel; the code of P_j of every block the call completed, from the signal ring into the code ring
// [block mod CB][N] uint16.  The discriminator's entry of the drain table covers it as it covers the ingest kernel
// (frame_signal.hip, "Why the stage has no entry of its own").
//
// occ_cover_kernel, one launch per I/Q-type call behind the frame_signal launch on K3's stream: lane = frame record of
// this call, grid-stride.  It stores 1 into the cover ring [block mod CB][N] uint8 for the blocks of the record's cover
// span (occupancy.h): same-value byte stores, so two frames over one block need no atomic.  Blocks in front of the run's
// first whole block belong to no epoch and are left alone: nobody would clear them.
//
// occ_epoch_kernel, one launch per final epoch behind the cover launch: a workgroup of four waves takes 64 channels, lane =
// channel, each wave a contiguous quarter of the epoch.  First pass: the histogram of the epoch's codes in LDS, [bin][32]
// words, lanes l and l + 32 in the two halves of a word (a count is at most E <= 4096; the two lanes are in different
// halves of the wave, so a wave's LDS add meets no bank twice), then the walk to rank floor(E / 8): every wave sums its 72
// bins, the wave whose bins hold the rank walks them.  Second pass: busy, covered and bursts with the floor known; the
// word (code | busy << 14 | cover << 15) goes back into the code ring, the cover bytes are cleared for the ring's next
// round, the last block's busy bit is carried to the next epoch.  The bit in front of a wave's quarter comes from the code
// of the block before it, read in the first pass (the second pass rewrites that word; its low nine bits stay).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "occupancy.h"

namespace gnuais {

namespace {

constexpr int OCC_THREADS = 256;
constexpr int OCC_LANES = 64;               // channels of a finaliser workgroup
constexpr int OCC_WAVES = OCC_THREADS / OCC_LANES;
constexpr int OCC_WAVE_BINS = OCC_BINS / OCC_WAVES;
constexpr int OCC_MAX_BLOCKS = 1024;        // grid-stride beyond that
constexpr int OCC_AHEAD = 8;                // blocks of n a thread of the finaliser has in flight
constexpr int OCC_HIST_WORDS = OCC_BINS * 32;
// hist | the waves' bin sums [4][64] | floor [64] | the waves' counts [3][4][64]
constexpr int OCC_LDS_WORDS = OCC_HIST_WORDS + OCC_THREADS + OCC_LANES + 3 * OCC_THREADS;
static_assert(OCC_BINS % OCC_WAVES == 0, "a wave's share of the bins");

HIP_DYNAMIC_SHARED(uint32_t, occ_lds)       // OCC_LDS_WORDS at the finaliser's launch

// grid: 1-D, block b = (block-of-n group b / n_groups, channel group b % n_groups); a thread walks the blocks of n of its
// group with stride `stride` = the number of groups
__global__ __launch_bounds__(OCC_THREADS) void occ_code_kernel(const int64_t *__restrict__ sums, int RB,
                                                               uint16_t *__restrict__ codes, int CB, int N, long long j0,
                                                               int count, int n_groups, int stride)
{
    const int grp = (int) (blockIdx.x % (unsigned) n_groups);
    const int c = grp * OCC_THREADS + (int) threadIdx.x;
    if (c >= N) return;
    for (int k = (int) (blockIdx.x / (unsigned) n_groups); k < count; k += stride) {
        const long long j = j0 + k;
        const int64_t P = sums[((size_t) (j % RB) * (size_t) N + (size_t) c) * 3];
        codes[(size_t) (j % CB) * (size_t) N + (size_t) c] = (uint16_t) occ_code(P);
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occ_cover_kernel(
    const uint32_t *__restrict__ frames, const uint32_t *__restrict__ frame_count, uint32_t frame_cap,
    const long long *__restrict__ times, uint8_t *__restrict__ cover, int CB, int N, long long n0, int len, uint32_t pllinc,
    int n_taps, int afc_window, long long v0, long long b0)
{
    const uint32_t cnt = frame_count[0];
    const uint32_t have = cnt < frame_cap ? cnt : frame_cap;
    for (uint32_t i = blockIdx.x * OCC_THREADS + threadIdx.x; i < have; i += gridDim.x * OCC_THREADS) {
        const long long t = times[i];
        if (t < n0 || t >= n0 + (long long) len) continue;      // another call's, or no time
        const uint32_t *rec = frames + (size_t) i * 16;
        const uint32_t c = rec[0];
        long long j_lo;
        int nb;
        if (c >= (uint32_t) N || !occ_cover_span(t, (int) (rec[15] >> 16), pllinc, n_taps, afc_window, v0, &j_lo, &nb)) continue;
        const long long end = j_lo + nb;
        if (end - j_lo >= CB) continue;                          // the host sized the ring beyond the longest span
        long long j = j_lo < b0 ? b0 : j_lo;
        int slot = (int) (j % (long long) CB);
        for (; j < end; ++j) {
            cover[(size_t) slot * (size_t) N + (size_t) c] = 1;
            if (++slot == CB) slot = 0;
        }
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occ_epoch_kernel(uint16_t *__restrict__ codes, uint8_t *__restrict__ cover,
                                                                uint8_t *__restrict__ carry, uint2 *__restrict__ out, int CB,
                                                                int N, int E, int margin, long long first, int first_epoch)
{
    uint32_t *hist = occ_lds, *part = hist + OCC_HIST_WORDS, *floor_s = part + OCC_THREADS, *cnt = floor_s + OCC_LANES;
    const int t = (int) threadIdx.x, lane = t & (OCC_LANES - 1), w = t / OCC_LANES;
    const int c = (int) blockIdx.x * OCC_LANES + lane;
    const bool live = c < N;
    const size_t col = live ? (size_t) c : 0;
    const int lo = (int) ((long long) E * w / OCC_WAVES), hi = (int) ((long long) E * (w + 1) / OCC_WAVES);
    const int slot_lo = (int) ((first + lo) % (long long) CB);
    const int word = lane & 31, shift = 16 * (lane >> 5);

    for (int i = t; i < OCC_HIST_WORDS; i += OCC_THREADS) hist[i] = 0;
    if (t < OCC_LANES) floor_s[t] = 0;
    // the code, or the carried bit, in front of this wave's quarter
    uint32_t before_code = 0, before_busy = 0;
    if (live && w > 0) before_code = codes[(size_t) ((first + lo - 1) % (long long) CB) * (size_t) N + col] & OCC_CODE_MASK;
    if (live && w == 0 && !first_epoch) before_busy = carry[col] != 0;
    __syncthreads();

    if (live) {
        // OCC_AHEAD blocks' codes are loaded before the first is counted: a lane's loads are N words apart, and one
        // load per LDS add leaves the memory pipe idle for its whole latency
        int slot = slot_lo;
        for (int k = lo; k < hi; k += OCC_AHEAD) {
            uint32_t code[OCC_AHEAD];
#pragma unroll
            for (int u = 0; u < OCC_AHEAD; ++u) {
                code[u] = OCC_BINS;
                if (k + u < hi) {
                    code[u] = codes[(size_t) slot * (size_t) N + col] & OCC_CODE_MASK;
                    if (++slot == CB) slot = 0;
                }
            }
#pragma unroll
            for (int u = 0; u < OCC_AHEAD; ++u) {
                if (k + u < hi) {
                    const uint32_t bin = code[u] < (uint32_t) OCC_BINS ? code[u] : (uint32_t) OCC_BINS - 1;
                    atomicAdd(&hist[bin * 32 + word], 1u << shift);
                }
            }
        }
    }
    __syncthreads();

    uint32_t mine = 0;
    for (int b = w * OCC_WAVE_BINS; b < (w + 1) * OCC_WAVE_BINS; ++b) mine += (hist[b * 32 + word] >> shift) & 0xffffu;
    part[w * OCC_LANES + lane] = mine;
    __syncthreads();
    {
        uint32_t acc = 0;
        for (int v = 0; v < w; ++v) acc += part[v * OCC_LANES + lane];
        const uint32_t rank = (uint32_t) (E / 8);
        if (acc <= rank && rank < acc + mine) {
            for (int b = w * OCC_WAVE_BINS; b < (w + 1) * OCC_WAVE_BINS; ++b) {
                acc += (hist[b * 32 + word] >> shift) & 0xffffu;
                if (acc > rank) {
                    floor_s[lane] = (uint32_t) b;
                    break;
                }
            }
        }
    }
    __syncthreads();

    const uint32_t floor_code = floor_s[lane], thr = floor_code + (uint32_t) margin;
    uint32_t busy = 0, covered = 0, bursts = 0;
    if (live) {
        uint32_t prev = w == 0 ? before_busy : (uint32_t) (before_code >= thr);
        int slot = slot_lo;
        for (int k = lo; k < hi; k += OCC_AHEAD) {
            // as many blocks' words before the first is rewritten: the ring is read and written through one pointer, so
            // the compiler keeps a load behind every store in front of it
            size_t idx[OCC_AHEAD];
            uint32_t code[OCC_AHEAD], cv[OCC_AHEAD];
#pragma unroll
            for (int u = 0; u < OCC_AHEAD; ++u) {
                idx[u] = (size_t) slot * (size_t) N + col;
                if (k + u < hi) {
                    code[u] = codes[idx[u]] & OCC_CODE_MASK;
                    cv[u] = cover[idx[u]] != 0;
                    if (++slot == CB) slot = 0;
                }
            }
#pragma unroll
            for (int u = 0; u < OCC_AHEAD; ++u) {
                if (k + u < hi) {
                    const uint32_t bz = code[u] >= thr;
                    busy += bz;
                    covered += bz & cv[u];
                    bursts += bz & (prev ^ 1u);
                    prev = bz;
                    codes[idx[u]] = (uint16_t) (code[u] | bz << OCC_BUSY_BIT | cv[u] << OCC_COVER_BIT);
                    if (cv[u]) cover[idx[u]] = 0;
                }
            }
        }
        if (w == OCC_WAVES - 1) carry[col] = (uint8_t) prev;
    }
    cnt[(0 * OCC_WAVES + w) * OCC_LANES + lane] = busy;
    cnt[(1 * OCC_WAVES + w) * OCC_LANES + lane] = covered;
    cnt[(2 * OCC_WAVES + w) * OCC_LANES + lane] = bursts;
    __syncthreads();
    if (w == 0 && live) {
        uint32_t s[3];
        for (int q = 0; q < 3; ++q) {
            s[q] = 0;
            for (int v = 0; v < OCC_WAVES; ++v) s[q] += cnt[(q * OCC_WAVES + v) * OCC_LANES + lane];
        }
        // gnuais_occupancy: uint16 floor, busy, covered, bursts
        out[col] = make_uint2(floor_code | s[0] << 16, s[1] | s[2] << 16);
    }
}

} // namespace

hipError_t launch_occ_code(const int64_t *sums, int RB, uint16_t *codes, int CB, int N, long long j0, int count,
                           hipStream_t stream)
{
    if (!sums || !codes || N <= 0 || RB <= 0 || CB <= 0 || j0 < 0 || count < 0 || count > RB || count > CB)
        return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    const int n_groups = (N + OCC_THREADS - 1) / OCC_THREADS;
    const int stride = count < OCC_MAX_BLOCKS ? count : OCC_MAX_BLOCKS;
    const long long blocks = (long long) n_groups * stride;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(occ_code_kernel, dim3((unsigned) blocks), dim3(OCC_THREADS), 0, stream, sums, RB, codes, CB, N, j0, count,
                       n_groups, stride);
    return hipGetLastError();
}

hipError_t launch_occ_cover(const OccCoverLaunch &a, hipStream_t stream)
{
    if (!a.frames || !a.frame_count || !a.times || !a.cover || a.N <= 0 || a.CB <= 0 || a.pllinc == 0 || a.n0 < 0 || a.len <= 0)
        return hipErrorInvalidValue;
    const unsigned want = (a.frame_cap + OCC_THREADS - 1) / OCC_THREADS;
    const unsigned blocks = want < 1u ? 1u : want > (unsigned) OCC_MAX_BLOCKS ? (unsigned) OCC_MAX_BLOCKS : want;
    hipLaunchKernelGGL(occ_cover_kernel, dim3(blocks), dim3(OCC_THREADS), 0, stream, (const uint32_t *) a.frames, a.frame_count,
                       a.frame_cap, (const long long *) a.times, a.cover, a.CB, a.N, (long long) a.n0, a.len, a.pllinc,
                       a.n_taps, a.afc_window, (long long) a.v0, (long long) a.b0);
    return hipGetLastError();
}

hipError_t launch_occ_epoch(const OccEpochLaunch &a, hipStream_t stream)
{
    if (!a.codes || !a.cover || !a.carry || !a.out || a.N <= 0 || a.E < OCC_MIN_EPOCH || a.E > OCC_MAX_EPOCH || a.CB <= a.E ||
        a.margin < 1 || a.margin > 255 || a.first < 0)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned) ((a.N + OCC_LANES - 1) / OCC_LANES);
    hipLaunchKernelGGL(occ_epoch_kernel, dim3(blocks), dim3(OCC_THREADS), sizeof(uint32_t) * OCC_LDS_WORDS, stream, a.codes,
                       a.cover, a.carry, (uint2 *) a.out, a.CB, a.N, a.E, a.margin, (long long) a.first, (int) a.first_epoch);
    return hipGetLastError();
}

} // namespace gnuais
