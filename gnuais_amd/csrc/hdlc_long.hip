// hdlc_long.hip -- the long-frame deframer D' for gfx950: AIS messages of three to five slots (definition:
// include/gnuais_hip.h, gnuais_batch_long_frames).
//
// D' is a second decoder per channel, independent of the chain's own (hdlc_events.hip / hdlc_crc.hip, which are not
// touched): protodec_decode() / protodec_reset() / protodec_calculate_crc() (src/protodec.c:988-1122, 87-100, 106-167)
// with the give-up test at 1031 stored bits instead of 449, delivering only what the chain's decoder cannot: frames of
// more than 426 bits whose CRC holds.  One launch per call, behind that call's K3 and in front of the event that frees
// the call's hand-off set (segbits / segcnt), only while the feature is on.
//
// Shape: lane = channel, 64 channels per wave, the machine's state in registers, every stream channel-contiguous
// (DESIGN section 3).  The walk is hdlc_deframe_kernel's "window by window" walk (hdlc_crc.hip), restated here:
//   ST_SKURR : "15 alternations then a 0" as a run-length test on x ^ (x << 1), up to 32 bits per step;
//   ST_DATA  : up to 32 RAW bits per step; the end of the frame (five 1s and a sixth) and the stored count (stuffed
//              0s counted with a popcount) are all that matter while a frame is open.  The raw bits go to the
//              channel's ONE open record, [LONG_REC_WORDS][N] words -- 1030 stored bits and at most 206 stuffed 0s --
//              which carries from call to call and restarts at every entry to ST_DATA;
//   ST_PREAMBLE / ST_STARTSIGN / ST_STOPSIGN bit by bit, but inside one step.
// The bit count is the chain's deframer's: ctl[2] / ctl[5] AFTER this call (that deframer ran in front of K3) less the
// bits of the call's packs, so a stamp is what that deframer gives a frame closing on the same bit, whenever the
// feature was switched on and wherever gnuais_batch_set_clock put the count.
//
// Closing a frame.  Long frames are rare (a few per minute and channel at most), so the lane that closes one with
// n > 426 does the rest itself, inside the walk: it unstuffs its open record in place (a thread reads back its own
// stores in program order; word ow of the result is written after raw word q >= ow was read), runs the reference's CRC
// over n/8 + 2 bytes of it, and appends the 152-byte record to the long ring through one atomic.  The other lanes of
// its wave wait for that -- a few microseconds where a long frame exists, nothing where none does -- which was chosen
// over a compact list and a second launch: one launch less in every call, and no list to size.
// While the repair of long frames is on (gnuais_batch_long_repair) the kernel runs in a second compile-time form that
// unstuffs into a record beside the open one and lists the frames whose CRC fails with their raw bits; see the kernel.
// The receive time needs nothing from outside either: the lane knows the segment s, the slice j, the segment's rows
// l_s and its bit count c_s of the closing bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gnuais {

namespace {

enum { LST_SKURR = 1, LST_PREAMBLE = 2, LST_STARTSIGN = 3, LST_DATA = 4, LST_STOPSIGN = 5 };

// lctl[0]: state[2:0] nstartsign[6:3] antallpreamble[10:7] antallenner[13:11] bitstuff[14] last[15] bufferpos[26:16]
// lctl[1]: partially filled word of the open record
// lctl[2]: raw bits in the open record
constexpr int LPACK_MAX = PACK_STRIDE;  // words per segment pack held in registers / LDS

__device__ __forceinline__ uint32_t l_lowmask(int k)    // k in [0, 32]
{
    return k >= 32 ? ~0u : ((1u << k) - 1u);
}
__device__ __forceinline__ int l_ctz32(uint32_t v)      // 32 for v == 0
{
    return v ? __ffs((int) v) - 1 : 32;
}
__device__ __forceinline__ int l_clz32(uint32_t v)      // 32 for v == 0
{
    return v ? __clz((int) v) : 32;
}

} // namespace

// everything of D' back to protodec_reset()'s state (protodec.c:87-100); counters: also the three counters
__global__ void hdlc_long_reset_kernel(uint32_t *__restrict__ lctl, int32_t *__restrict__ counters, int N)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    lctl[c] = LST_SKURR;
    lctl[(size_t) N + c] = 0;
    lctl[(size_t) 2 * N + c] = 0;
    if (counters) {
        counters[c] = 0;
        counters[(size_t) N + c] = 0;
        counters[(size_t) 2 * N + c] = 0;
    }
}

HIP_DYNAMIC_SHARED(uint32_t, long_pack)                     // [LPACK_MAX + 1][blockDim.x]

// The kernel in its two compile-time forms.  KEEP_RAW = false is D' as gnuais_batch_long_frames defines it and is what
// runs while the repair of long frames is off: its last five arguments are not read.  KEEP_RAW = true (gnuais_batch_long_repair) keeps what that form destroys:
// the unstuffed bits go to a second per-channel record, `clean`, so `open` still holds the raw bits when the CRC fails,
// and the lane then appends one candidate record (kernels.h: LONG_CAND_*) to the candidate ring through one atomic on
// cand_count[parity].  It also clears cand_count[parity ^ 1], the counter of the NEXT call: the two are used by call
// parity, and the repair launch that read the other one ran in front of this launch.
template <bool KEEP_RAW = false>
__global__ __launch_bounds__(64) void hdlc_long_kernel(
    const uint32_t *__restrict__ segbits, const uint32_t *__restrict__ segcnt, const uint32_t *__restrict__ ctl,
    uint32_t *__restrict__ lctl, uint32_t *open, int32_t *__restrict__ counters, uint32_t *__restrict__ frames,
    uint32_t *__restrict__ frame_count, uint32_t frame_cap, int N, int n_seg, int seg_words, int len, long long n0,
    uint32_t *clean = nullptr, uint32_t *__restrict__ cand = nullptr, uint32_t *cand_count = nullptr,
    uint32_t cand_cap = 0, int parity = 0)
{
    uint32_t *const urec = KEEP_RAW ? clean : open;             // where the unstuffed bits of a closing frame go
    if (KEEP_RAW && blockIdx.x == 0 && threadIdx.x == 0) cand_count[parity ^ 1] = 0;
    const int cg = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = cg < N;
    const size_t c = (size_t) (live ? cg : N - 1), n_ = (size_t) N;

    const uint32_t c0 = lctl[c];
    int state = c0 & 7, nstartsign = (c0 >> 3) & 15, antallpreamble = (c0 >> 7) & 15;
    int antallenner = (c0 >> 11) & 7, bitstuff = (c0 >> 14) & 1;
    uint32_t last = (c0 >> 15) & 1;
    int bufferpos = (c0 >> 16) & 2047;
    uint32_t cur = lctl[n_ + c];
    int rawpos = (int) lctl[2 * n_ + c];
    int delivered = 0, failed = 0;

    const int seg_cap = seg_words * 32;
    const uint32_t *__restrict__ cnts = segcnt + c * (size_t) n_seg;
    // bits fed before the current segment: the chain's deframer's count behind this call, less the call's bits
    unsigned long long seenbase = (unsigned long long) ctl[2 * n_ + c] | ((unsigned long long) ctl[5 * n_ + c] << 32);
    for (int s = 0; s < n_seg; ++s) {
        const int cs = live ? (int) cnts[s] : 0;
        seenbase -= (unsigned long long) (cs > seg_cap ? seg_cap : cs);
    }

#define LONG_RESET()                                                                    \
    do { state = LST_SKURR; nstartsign = 0; antallpreamble = 0; antallenner = 0;       \
         last = 0; bitstuff = 0; bufferpos = 0; } while (0)

    // the pack of the NEXT segment is fetched into registers while the current one is walked out of LDS
    const int tpb = (int) blockDim.x, tx = (int) threadIdx.x;
    const uint32_t *__restrict__ rows = segbits + c * (size_t) n_seg * (size_t) PACK_STRIDE;
    uint32_t pf[LPACK_MAX];
    int pf_cnt = live ? (int) cnts[0] : 0;
    // a pack is PACK_STRIDE words, 64-byte aligned, zero beyond its bits: four 16-byte loads
#pragma unroll
    for (int q = 0; q < LPACK_MAX / 4; ++q) {
        const uint4 v = reinterpret_cast<const uint4 *>(rows)[q];
        pf[4 * q] = v.x; pf[4 * q + 1] = v.y; pf[4 * q + 2] = v.z; pf[4 * q + 3] = v.w;
    }

    for (int seg = 0; seg < n_seg; ++seg) {
        int tile_end = pf_cnt;
        if (tile_end > seg_cap) tile_end = seg_cap;
#pragma unroll
        for (int q = 0; q < LPACK_MAX; ++q) long_pack[q * tpb + tx] = pf[q];
        long_pack[LPACK_MAX * tpb + tx] = 0;
        if (seg + 1 < n_seg) {
            const uint32_t *__restrict__ nrow = rows + (size_t) (seg + 1) * (size_t) PACK_STRIDE;
            pf_cnt = live ? (int) cnts[seg + 1] : 0;
#pragma unroll
            for (int q = 0; q < LPACK_MAX / 4; ++q) {
                const uint4 v = reinterpret_cast<const uint4 *>(nrow)[q];
                pf[4 * q] = v.x; pf[4 * q + 1] = v.y; pf[4 * q + 2] = v.z; pf[4 * q + 3] = v.w;
            }
        }
        int pos = 0;
        // the walk is batched by mode, as in hdlc_deframe_kernel: an iteration runs exactly one mode's code
#define FETCH_WINDOW()                                                                          \
        const int lw = pos >> 5, sh = pos & 31;                                                 \
        const uint32_t lo = long_pack[lw * tpb + tx], hi = long_pack[(lw + 1) * tpb + tx];      \
        const uint32_t W = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo; /* bit j = x[pos+j] */  \
        const int nv = (tile_end - pos < 32) ? tile_end - pos : 32

        while (__any(pos < tile_end)) {
            // ---- ST_SKURR: protodec.c:1030-1043, up to 32 bits per step -------------
            while (__any(pos < tile_end && state == LST_SKURR)) {
                if (pos < tile_end && state == LST_SKURR) {
                    FETCH_WINDOW();
                    const uint32_t vm = l_lowmask(nv);
                    const uint32_t A = W ^ ((W << 1) | last);      // bit j: x_j != x_{j-1}
                    const uint32_t B2 = A & (A << 1), B4 = B2 & (B2 << 2), B8 = B4 & (B4 << 4);
                    const uint32_t B15 = B8 & (B8 << 7);           // 15 alternations inside the window
                    const int t = l_ctz32(~A);                      // alternation run from the window start
                    const int need = 14 - antallpreamble;           // run continues the carried count
                    const uint32_t C = l_lowmask(t) & ~l_lowmask(need > 0 ? need : 0);
                    const uint32_t TR = (B15 | C) & ~W & vm;        // antallpreamble > 14 && x == 0
                    if (TR) {
                        pos += l_ctz32(TR) + 1;
                        state = LST_PREAMBLE;
                        antallpreamble = 0;
                        last = 0;
                    } else {
                        pos += nv;
                        last = (W >> (nv - 1)) & 1u;
                        const int ap = (t >= nv) ? antallpreamble + nv : l_clz32(~(A << (32 - nv)));
                        antallpreamble = ap > 15 ? 15 : ap;
                    }
                }
            }
            // ---- ST_PREAMBLE / ST_STARTSIGN / ST_STOPSIGN: protodec.c:1045-1115 ----------
            // From PREAMBLE with nstartsign = k >= 1 (or STARTSIGN, k = 6, 7) the machine needs R = 7 - k more 1s and
            // then a 0 to enter ST_DATA; a 0 among the first R-1 of them resets from PREAMBLE (nstartsign 0), a 0 at
            // the R-th or a 1 after them resets from STARTSIGN (nstartsign 1 after its trailing ++).
            while (__any(pos < tile_end && state != LST_SKURR && state != LST_DATA)) {
                if (pos < tile_end && state != LST_SKURR && state != LST_DATA) {
                    FETCH_WINDOW();
                    int k = 0;
                    if (state == LST_STOPSIGN) {                // protodec.c:1095-1115
                        const uint32_t x = W & 1u;
                        const int nb = bufferpos - 6 - 16;
                        if (x == 0 && nb > LONG_SHORT_BITS) {   // a long frame: the rest is this lane's own work
                            const int last_w = rawpos >> 5;
                            if (last_w < LONG_REC_WORDS) open[(size_t) last_w * n_ + c] = cur;
                            // protodec.c:1008-1023 on the raw bits, in place: every bit except the 0 that follows
                            // five 1s (inside a frame a run of 1s is at most five long: a sixth closed it)
                            {
                                unsigned long long acc = 0;
                                uint32_t prevw = 0;
                                int fill = 0, ow = 0;
                                const int nwords = (rawpos + 31) >> 5 < LONG_REC_WORDS ? (rawpos + 31) >> 5 : LONG_REC_WORDS;
#pragma unroll 1
                                for (int q = 0; q < nwords; ++q) {
                                    uint32_t rw = open[(size_t) q * n_ + c];
                                    const int nvq = rawpos - 32 * q < 32 ? rawpos - 32 * q : 32;
                                    const unsigned long long cc = ((unsigned long long) rw << 32) | prevw;
                                    const uint32_t five = (uint32_t) (cc >> 31) & (uint32_t) (cc >> 30) & (uint32_t) (cc >> 29) &
                                                          (uint32_t) (cc >> 28) & (uint32_t) (cc >> 27);
                                    uint32_t stf = five & ~rw & l_lowmask(nvq);
                                    prevw = rw;
                                    int nout = nvq;
                                    while (stf) {               // highest first: lower positions stay valid
                                        const int pz = 31 - __clz((int) stf);
                                        stf &= ~(1u << pz);
                                        rw = (rw & ((1u << pz) - 1u)) | ((pz >= 31 ? 0u : rw >> (pz + 1)) << pz);
                                        --nout;
                                    }
                                    rw &= l_lowmask(nout);
                                    acc |= (unsigned long long) rw << fill;
                                    fill += nout;
                                    if (fill >= 32) {           // ow <= q: behind the word just read
                                        urec[(size_t) ow * n_ + c] = (uint32_t) acc;
                                        ++ow;
                                        acc >>= 32;
                                        fill -= 32;
                                    }
                                }
                                if (ow < LONG_REC_WORDS) urec[(size_t) ow * n_ + c] = (uint32_t) acc;
                            }
                            // protodec_calculate_crc(nb): protodec_sdlc_crc() over nb/8 + 2 bytes, bits LSB first
                            const int nbytes = nb >> 3, buflen = nbytes + 2;
                            uint32_t crc = 0xffffu;
#pragma unroll 1
                            for (int q = 0; q * 4 < buflen; ++q) {
                                const uint32_t w = urec[(size_t) q * n_ + c];
                                const int nby = buflen - q * 4 < 4 ? buflen - q * 4 : 4;
#pragma unroll 1
                                for (int bq = 0; bq < nby; ++bq) {
                                    crc ^= (w >> (8 * bq)) & 0xffu;
#pragma unroll
                                    for (int i = 0; i < 8; ++i) crc = (crc >> 1) ^ ((crc & 1u) ? 0x8408u : 0u);
                                }
                            }
                            // the stamp: bits fed before the closing bit, as the chain's deframer counts them; the time:
                            // -1 for bits without samples (gnuais_batch_decode_bits)
#define LONG_STAMP_AND_TIME()                                                                                           \
                                    const unsigned long long eb = seenbase + (unsigned long long) pos;                  \
                                    long long t = -1;                                                                   \
                                    if (len > 0) {                                                                      \
                                        const long long ls = len - seg * SEG_LEN < SEG_LEN ? len - seg * SEG_LEN : SEG_LEN; \
                                        t = n0 + (long long) seg * SEG_LEN + ((2 * (long long) pos + 1) * ls) / (2 * (long long) tile_end); \
                                    }
                            if (crc == 0xf0b8u) {               // ~crc == 0x0f47, protodec.c:166
                                ++delivered;
                                const uint32_t slot = atomicAdd(&frame_count[0], 1u);
                                if (slot < frame_cap) {
                                    LONG_STAMP_AND_TIME()
                                    uint32_t *dst = frames + (size_t) slot * LONG_FRAME_WORDS;
                                    dst[0] = (uint32_t) c;
                                    dst[1] = (uint32_t) eb;
                                    dst[2] = (uint32_t) (unsigned long long) t;
                                    dst[3] = (uint32_t) ((unsigned long long) t >> 32);
                                    dst[4] = (uint32_t) nb | ((1u | (((uint32_t) (eb >> 32) & 31u) << 1)) << 16);
#pragma unroll 1
                                    for (int q = 0; q < LONG_FRAME_WORDS - 5; ++q) {
                                        uint32_t v = 0;
                                        if (q * 4 < nbytes) {
                                            v = urec[(size_t) q * n_ + c];
                                            const int keep = nbytes - q * 4;
                                            if (keep < 4) v &= (1u << (8 * keep)) - 1u;
                                        }
                                        dst[5 + q] = v;
                                    }
                                } else {
                                    frame_count[1] = 1;         // ring full: frame dropped, still counted
                                }
                            } else {
                                ++failed;
                                if (KEEP_RAW) {                 // a candidate of the repair: the record as it was received
                                    const uint32_t slot = atomicAdd(&cand_count[parity], 1u);
                                    if (slot < cand_cap) {      // sized so that every close of one call fits
                                        LONG_STAMP_AND_TIME()
                                        uint32_t *dst = cand + (size_t) slot * LONG_CAND_WORDS;
                                        dst[0] = (uint32_t) c;
                                        dst[1] = (uint32_t) eb;
                                        dst[2] = (uint32_t) (unsigned long long) t;
                                        dst[3] = (uint32_t) ((unsigned long long) t >> 32);
                                        dst[4] = (uint32_t) nb | (((uint32_t) (eb >> 32) & 31u) << 16);
                                        dst[5] = (uint32_t) rawpos;
                                        const int nwords = (rawpos + 31) >> 5 < LONG_REC_WORDS ? (rawpos + 31) >> 5 : LONG_REC_WORDS;
#pragma unroll 1
                                        for (int q = 0; q < LONG_REC_WORDS; ++q)
                                            dst[LONG_CAND_HDR + q] = q < nwords ? open[(size_t) q * n_ + c] : 0u;
                                    }
                                }
                            }
#undef LONG_STAMP_AND_TIME
                        }
                        // nb <= 426, a stop bit of 1, nb <= 0: the chain's decoder's business; D' says nothing
                        LONG_RESET();
                        last = x;                               // protodec.c:1119
                        k = 1;
                    } else if (state != LST_PREAMBLE && state != LST_STARTSIGN) {
                        LONG_RESET();                           // not a state: as the reference's
                        last = W & 1u;                          // switch would fall through
                        k = 1;
                    } else {
                        if (state == LST_PREAMBLE && nstartsign == 0) {
                            // alternating part of the training sequence, all at once
                            const uint32_t A = W ^ ((W << 1) | last);
                            int t = l_ctz32(~A);
                            if (t > nv) t = nv;
                            if (t > 0) {
                                antallpreamble = antallpreamble + t > 15 ? 15 : antallpreamble + t;
                                last = (W >> (t - 1)) & 1u;
                                k = t;
                            }
                            if (k < nv) {                       // first repeated bit
                                const uint32_t x0 = (W >> k) & 1u;
                                nstartsign = x0 ? 3 : 1;        // protodec.c:1052-1053 / 1065-1066
                                last = x0;
                                ++k;
                            }
                        }
                        if (k < nv && nstartsign != 0) {
                            const int R = 7 - nstartsign;       // 1s still needed, then a 0
                            const int avail = nv - k;
                            int L = l_ctz32(~(W >> k));         // run of 1s from bit k
                            if (L > avail) L = avail;
                            if (L >= R + 1) {                   // a 1 where the 0 had to be
                                LONG_RESET(); nstartsign = 1; last = 1; k += R + 1;
                            } else if (L < avail) {             // the run ends on a visible 0
                                if (L == R) {                   // protodec.c:1076-1082: ST_DATA, the open record restarts
                                    state = LST_DATA; nstartsign = 1; antallenner = 0; antallpreamble = 0;
                                    bufferpos = 0; cur = 0; rawpos = 0; bitstuff = 0; last = 0;
                                } else if (L == R - 1) {        // 0 in ST_STARTSIGN (nstartsign 6)
                                    LONG_RESET(); nstartsign = 1; last = 0;
                                } else {                        // 0 while still in ST_PREAMBLE
                                    LONG_RESET(); last = 0;
                                }
                                k += L + 1;
                            } else {                            // only 1s left in this window
                                nstartsign += L;
                                if (nstartsign >= 6) { state = LST_STARTSIGN; antallpreamble = 0; }
                                last = 1;
                                k += L;
                            }
                        }
                    }
                    pos += k;
                }
            }
            // ---- ST_DATA: protodec.c:995-1028, up to 32 raw bits per step ----------------
            while (__any(pos < tile_end && state == LST_DATA)) {
                if (pos < tile_end && state == LST_DATA) {
                    FETCH_WINDOW();
                    if (bitstuff) {                             // protodec.c:996-1007
                        const uint32_t x = W & 1u;
                        if (x) {
                            state = LST_STOPSIGN;               // sixth 1: closing flag (or abort)
                        } else {                                // stuffed 0: stays in the raw record
                            if ((rawpos & 31) == 31) {
                                if ((rawpos >> 5) < LONG_REC_WORDS) open[(size_t) (rawpos >> 5) * n_ + c] = cur;
                                cur = 0;
                            }
                            ++rawpos;
                        }
                        bitstuff = 0;
                        last = x;
                        pos += 1;
                    } else {                                    // protodec.c:1008-1027
                        // m = run of 1s ending at the previous bit (antallenner = m-1 when last = 1)
                        const int m = last ? antallenner + 1 : 0;
                        const int room = LONG_LIMIT_BITS - bufferpos;   // the give-up test of D'
                        int nw = nv;
                        if (nw > 32 - m) nw = 32 - m;
                        if (nw > room) nw = room;               // bufferpos can reach the limit only at
                                                                // the last bit of this step
                        const int nvE = nw + m;
                        const uint32_t vmE = l_lowmask(nvE);
                        // E: the carried 1s, then the window; bit j = raw bit j-m
                        const uint32_t E = ((W << m) | l_lowmask(m)) & vmE;
                        const uint32_t X1 = E & (E >> 1), X2 = X1 & (X1 >> 2);
                        const uint32_t R5 = X2 & (E >> 4);      // five 1s starting at bit j
                        const uint32_t S5 = R5 & ~(E << 1);     // ... that begin a run
                        const uint32_t P5 = S5 << 4;            // position of the run's fifth 1
                        const uint32_t nx = E >> 1, kn = vmE >> 1;
                        const uint32_t END5 = P5 & nx & kn;     // followed by a sixth 1: closing flag
                        const uint32_t STF5 = P5 & ~nx & kn;    // followed by a 0: stuffing, dropped
                        const uint32_t PND5 = P5 & ~kn;         // fifth 1 is the last bit seen
                        int nraw, stored;
                        if (END5) {
                            const int pe = l_ctz32(END5);
                            nraw = pe + 1 - m;                  // raw bits up to the fifth 1
                            stored = nraw - __popc(STF5 & l_lowmask(pe));
                        } else {
                            nraw = nw;
                            stored = nw - __popc(STF5);
                        }
                        {   // open record [rawpos .. rawpos+nraw) = x[pos .. pos+nraw)
                            const uint32_t sb = W & l_lowmask(nraw);
                            const int bsh = rawpos & 31;
                            const unsigned long long t64 = (unsigned long long) sb << bsh;
                            cur |= (uint32_t) t64;
                            if (bsh + nraw >= 32) {
                                if ((rawpos >> 5) < LONG_REC_WORDS) open[(size_t) (rawpos >> 5) * n_ + c] = cur;
                                cur = (uint32_t) (t64 >> 32);
                            }
                            rawpos += nraw;
                        }
                        bufferpos += stored;
                        if (END5) {
                            pos += nraw + 1;                    // ... and the sixth 1
                            state = LST_STOPSIGN;
                            antallenner = 0;
                            last = 1;
                        } else {
                            pos += nraw;
                            const uint32_t xl = (W >> (nraw - 1)) & 1u;
                            if (bufferpos >= LONG_LIMIT_BITS) { // give up the frame
                                LONG_RESET();
                                last = xl;
                            } else if (PND5) {                  // next bit is stuffing or flag
                                bitstuff = 1;
                                antallenner = 0;
                                last = 1;
                            } else {
                                const int r = l_clz32(~(E << (32 - nvE)));   // run of 1s at the end
                                last = xl;
                                antallenner = r > 0 ? r - 1 : 0;
                            }
                        }
                    }
                }
            }
        }
#undef FETCH_WINDOW
        seenbase += (unsigned long long) tile_end;
    }
#undef LONG_RESET

    if (live) {
        lctl[c] = (uint32_t) state | ((uint32_t) nstartsign << 3) | ((uint32_t) antallpreamble << 7) |
                  ((uint32_t) antallenner << 11) | ((uint32_t) bitstuff << 14) | (last << 15) |
                  ((uint32_t) bufferpos << 16);
        lctl[n_ + c] = cur;
        lctl[2 * n_ + c] = (uint32_t) rawpos;
        if (delivered) counters[c] += delivered;
        if (failed) counters[n_ + c] += failed;
    }
}

hipError_t launch_hdlc_long(const LongLaunch &a, hipStream_t stream)
{
    if (!a.segbits || !a.segcnt || !a.ctl || !a.lctl || !a.open || !a.counters || !a.frames || !a.frame_count ||
        a.N <= 0 || a.n_seg <= 0 || a.seg_words <= 0 || a.seg_words > LPACK_MAX || a.len > a.n_seg * SEG_LEN)
        return hipErrorInvalidValue;
    if (a.clean) {                              // the repair of long frames is on: the form that keeps the raw bits
        if (!a.cand || !a.cand_count || a.cand_cap == 0) return hipErrorInvalidValue;
        hipLaunchKernelGGL(hdlc_long_kernel<true>, dim3((a.N + 63) / 64), dim3(64), (LPACK_MAX + 1) * 64 * sizeof(uint32_t),
                           stream, a.segbits, a.segcnt, a.ctl, a.lctl, a.open, a.counters, (uint32_t *) a.frames,
                           a.frame_count, a.frame_cap, a.N, a.n_seg, a.seg_words, a.len, (long long) a.n0, a.clean, a.cand,
                           a.cand_count, a.cand_cap, a.parity);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(hdlc_long_kernel<false>, dim3((a.N + 63) / 64), dim3(64), (LPACK_MAX + 1) * 64 * sizeof(uint32_t), stream,
                       a.segbits, a.segcnt, a.ctl, a.lctl, a.open, a.counters, (uint32_t *) a.frames, a.frame_count,
                       a.frame_cap, a.N, a.n_seg, a.seg_words, a.len, (long long) a.n0, (uint32_t *) nullptr,
                       (uint32_t *) nullptr, (uint32_t *) nullptr, 0u, 0);
    return hipGetLastError();
}

hipError_t launch_hdlc_long_reset(uint32_t *lctl, int32_t *counters, int N, hipStream_t stream)
{
    hipLaunchKernelGGL(hdlc_long_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, lctl, counters, N);
    return hipGetLastError();
}

} // namespace gnuais
