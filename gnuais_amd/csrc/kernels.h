// kernels.h -- internal launch interface between the C-ABI host code
// (gnuais_capi.hip, capi_ingest.hip, capi_delivery.hip over batch.h) and the gfx950 kernels.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fir_plan.h"   // what the host decides before a FIR launch: the slicer's bounds, the kernel, T's quanta (no HIP in there)

namespace gnuais {

// ---- K1: FIR + slicer (fir_slice.hip) -------------------------------------
struct FirLaunch : FirThresholds {   // NC, T, eps .. eps_ahead_k: the host's decision (fir_plan.h)
    const int16_t *x;      // [L][N] interleaved input
    const int16_t *hist;   // [NT][N] previous call's last NT samples, oldest first
    uint32_t *sgn;         // sign words, bit 31 = oldest sample; layout: sgn_index() below
    float *dump;           // optional [L][N] filter output
    int *maxval;           // [N] peak positive sample (atomicMax into a zeroed buffer)
    int16_t *hist_out;     // [NT][N] the other history buffer: written by the specialised kernel
    int *maxval_next;      // [N] the other peak buffer: cleared by the specialised kernel
    const float *d_taps;   // device copy of all NT taps (generic kernel)
    float te[64];          // trimmed taps (specialised kernel)
    int N, L;
    int NT, NE, d;         // out[n] = sum_j te[j] * x[n - d + j], j < NE
    float ctaps[48];       // the NC central taps, te[(NE-NC)/2 .. +NC)
    const float *te_mem;   // the NE effective taps in device memory (exact re-evaluation)
    int map;               // K1s workgroup -> (channel group, segment) mapping, see fir_sign_kernel
    int max_segments = 0;  // fir_sign_pk.hip: > 0 = only the call's first segments (the rest is fir_sign_mfma.hip's)
    const struct MfmaTaps *mfma = nullptr;   // fir_sign_mfma.hip: the device copy of its integer taps; eps_seen / eps_ahead are then in ITS units
};
int launch_fir_sign_quantum(int NC);           // T must be a multiple of this
hipError_t launch_fir_sign(const FirLaunch &a, hipStream_t stream);
// K1s in transposed form on register pairs (fir_sign_pk.hip): NC 12 (32-tap table), 40 or 48
int launch_fir_sign_pk_quantum(int NC);
// K1s, 48 central taps as an exact integer Toeplitz product on the matrix pipe (fir_sign_mfma.hip): outputs first .. of a call
struct alignas(16) MfmaTaps { int a[3][3][64][4]; int k0; };   // [block of 32 window rows][tap digit 0..2][lane][16 bytes]: the A operands; 128 * sum of the integer taps
void fir_sign_mfma_pack(const int *tq48, long tq_sum, MfmaTaps *out);     // SignBounds::tq, ::tq_sum -> the A operands
hipError_t launch_fir_sign_mfma(const FirLaunch &a, int first, hipStream_t stream);
hipError_t launch_fir_sign_pk(const FirLaunch &a, hipStream_t stream);
hipError_t launch_fir_generic(const FirLaunch &a, hipStream_t stream);
hipError_t launch_fir_history(const int16_t *x, const int16_t *hist_in, int16_t *hist_out,
                              int N, int L, int NT, hipStream_t stream);

// ---- K2: PLL clock recovery, slice + NRZI (pll_h3.hip, pll_tp.hip) ----------------
constexpr int PLL_LDS_BYTES = 81 * 1024;   // > half of a CU's LDS: one PLL workgroup per CU
constexpr int SEG_WORDS = 64;        // segment (one bit pack per channel): 64 sign words
constexpr int SEG_LEN = SEG_WORDS * 32;    //   = 2048 samples
constexpr int PACK_STRIDE = 16;      // words reserved per (channel, segment) bit pack: 64 bytes
// Sign words: word w (samples 32w .. 32w+31, bit 31 = oldest) of channel c.  Four consecutive
// words of a channel lie side by side, so that K2 fetches 128 samples of a channel with one
// 16-byte load and a wave's fetch is 1 KB of contiguous memory.
__host__ __device__ inline size_t sgn_index(int w, int N, int c)
{
    return ((size_t) (w >> 2) * (size_t) N + (size_t) c) * 4 + (size_t) (w & 3);
}
__host__ __device__ inline size_t sgn_words_alloc(int W, int N)   // words for W sign words per channel
{
    return (size_t) ((W + 3) / 4 + 1) * 4 * (size_t) N;
}
struct PllLaunch {
    const uint32_t *sgn;   // sgn_index() layout
    uint32_t *pll;         // [N] phase (receiver.h:40), carried
    uint32_t *prev;        // [N] sign of the last sample (receiver.h:44), carried
    uint32_t *lastbit;     // [N] level at the last slice (receiver.h:38), carried
    uint32_t *watchdog;    // one word: set to 1 if a wave of the launch gave up waiting for its partner
    uint32_t *segbits;     // [N][n_seg][PACK_STRIDE] recovered bits per segment, LSB first
    uint32_t *segcnt;      // [N][n_seg] bits in each pack
    int N, L, n_seg, seg_words;
    uint32_t pllinc;
    int n_cu;              // compute units of the batch's device
    int variant = 0;       // 0: by channel count; 7: the time-parallel form (pll_tp.hip); 8: one recurrence wave + three helpers (pll_h3.hip)
};
int pll_form_of(const PllLaunch &a);                                     // the form launch_pll() will take: 7 or 8
int pll_need_lds();                                                      // bytes of LDS a PLL workgroup cannot do without
hipError_t pll_prepare_device();                                         // once per device, after hipSetDevice
hipError_t launch_pll(const PllLaunch &a, hipStream_t stream);           // K2
// K2 in its time-parallel form (pll_tp.hip): a workgroup per channel, lanes = candidate phases; small batches
bool pll_tp_applicable(const PllLaunch &a);
hipError_t launch_pll_tp(const PllLaunch &a, hipStream_t stream);
constexpr int PLL_TP_MAX_CHANNELS = 1536; // launch_pll() takes the time-parallel form by itself up to this many channels (48 000 samples: 0.066 / 0.118 / 0.219 / 0.423 ms at 512 / 1024 / 2048 / 4096 against pll_h3's 0.32)

// ---- K2b: HDLC deframer, K3: CRC-16 + frame delivery (hdlc_crc.hip) ---------
constexpr int HDLC_CTL_WORDS = 6;
constexpr int HDLC_BUF_WORDS = 15;   // 449 bits max (protodec.c:1024)
constexpr int CAND_HDR = 2;          // [0] nbits | valid flag | raw length << 17 | end_bit[36:32] << 27, [1] end_bit[31:0]
constexpr int CAND_WORDS = 20;       // header + 17 raw words (449 frame bits + stuffing) = 80 bytes
struct HdlcLaunch {
    const uint32_t *segbits;  // as above (PACK_STRIDE words per pack)
    const uint32_t *segcnt;
    uint32_t *ctl;         // [HDLC_CTL_WORDS][N] control state
    uint32_t *cand;        // [N][K][CAND_WORDS] per-channel ring of candidate frames
    uint32_t *cand_first;  // [N] first slot closed in this call
    uint32_t *cand_count;  // [N] slots closed in this call
    int32_t *counters;     // [3][N] receivedframes, lostframes, lostframes2
    void *frames;          // gnuais_frame[frame_cap]
    uint32_t *frame_count; // [4]: frames appended, overflow flag, -, PLL watchdog
    uint32_t frame_cap;
    int N, n_seg, seg_words, K;   // K: slots of a channel's candidate ring
    int K_call = 0;        // most frame starts one call can have (<= K; 0: K); sizes the chunk table
    int lanes_per_wave;    // channels per wave in K2b (blockDim)
    uint2 *chunks = nullptr;   // optional [blocks of K3][k3_passes(K)]: where each pass of each K3 block put its
                           // frames in the ring (start, count).  (block, pass, position) is the reference's
                           // print order -- channel, then time -- so a ring that holds ONE call needs no sort
    // gnuais_batch_discard_frames without a dispatch of its own: the deframer launch that carries `discard` empties the
    // ring's three words in front of its own K3 and behind the previous one (stream order), where the memset used to sit.
    // Other blocks of the same launch may already have marked a candidate that found no slot in word 1, so that mark is
    // the value `ovf_mark` (2 or 4: it changes with every discard-carrying launch; readers ask for non-zero) and the
    // clearing thread ANDs the word with it: whatever earlier launches left is gone (K3's 1, the other value), what this
    // launch says stays, in either order of the two accesses.  The kernels take both in one word: ovf_mark | discard.
    bool discard = false;
    uint32_t ovf_mark = 2;
};
#if defined(__HIPCC__)
__device__ __forceinline__ void hdlc_discard_ring(uint32_t *flags, uint32_t ovf_mark)
{
    flags[0] = 0;
    atomicAnd(&flags[1], ovf_mark);
    flags[2] = 0;
}
#endif
constexpr int K3_CH = 32;               // channels per K3 block
inline int k3_blocks(int N) { return (N + K3_CH - 1) / K3_CH; }
inline int k3_passes(int K) { return (K3_CH * K + 255) / 256; }
hipError_t launch_hdlc_deframe(const HdlcLaunch &a, hipStream_t stream); // K2b, window by window (hdlc_crc.hip)
hipError_t launch_hdlc_events(const HdlcLaunch &a, hipStream_t stream);  // K2b, event by event (hdlc_events.hip)
hipError_t launch_hdlc_crc(const HdlcLaunch &a, hipStream_t stream);     // K3
hipError_t launch_hdlc_reset(uint32_t *ctl, int N, hipStream_t stream);
hipError_t launch_hdlc_fsm_reset(uint32_t *ctl, int N, hipStream_t stream);   // protodec_reset() only: counters and time stay

// ---- the receive time of the frames K3 appended in one call (frame_time.hip; definition in include/gnuais_hip.h) ----
// One launch behind that call's K3, on its stream, before the call's hand-off set (segcnt) can be reused and before
// the next deframer launch moves ctl on.  Writes times[i] for every record i of the ring whose end_bit lies among the
// bits this call fed; other records are left alone.  len <= 0: the call fed bits without samples
// (gnuais_batch_decode_bits), its frames get -1.
struct FrameTimeLaunch {
    const void *frames;            // gnuais_frame[frame_cap]: the ring K3 appended to
    const uint32_t *frame_count;   // its counters ([0] = frames appended)
    uint32_t frame_cap;
    const uint32_t *ctl;           // the deframer's control state AFTER the call ([2], [5]: bits fed since reset)
    const uint32_t *segcnt;        // [N][n_seg] of the call's hand-off set
    int64_t *times;                // [frame_cap], by ring slot
    int N, n_seg, seg_words;
    int len;                       // rows of the call
    int64_t n0;                    // rows the chain had taken before it
};
hipError_t launch_frame_times(const FrameTimeLaunch &a, hipStream_t stream);
// times[order[j]] -> out[j], j < n: the times in the order of a sorted drain (frames_sort_timed)
hipError_t launch_frame_times_gather(const int64_t *times, const uint32_t *order, int n, int64_t *out, hipStream_t stream);

// ---- the signal power and carrier error of every frame (frame_signal.hip; definition in include/gnuais_hip.h) ----
// launch_iq_power: in front of the discriminator of an I/Q-type call, on its stream.  iq [len][N][2] int16 is what that
// discriminator reads; n0 = rows the chain had taken before the call; carry [N] words is the stage's own previous pair;
// ring [RB][N][3] int64 (P, R, I) holds block j of n in slot j % RB, RB >= len / 64 + 2.  first: the call starts a run of
// I/Q-type calls (n0 == v0): the previous pair is (0, 0) and the open block is set, not added to.
hipError_t launch_iq_power(const int16_t *iq, uint32_t *carry, int64_t *ring, int RB, int N, int len,
                           unsigned long long n0, bool first, hipStream_t stream);
// launch_frame_signal: behind the frame_time launch of the same call, on its stream.  Writes signal[i] for every record i
// of the ring with times[i] < 0 -- (0, 0, 0) -- or n0 <= times[i] < n0 + len; other records are left alone.
struct FrameSignalLaunch {
    const void *frames;            // gnuais_frame[frame_cap]: the ring K3 appended to
    const uint32_t *frame_count;   // its counters ([0] = frames appended)
    uint32_t frame_cap;
    const int64_t *times;          // [frame_cap], by ring slot (frame_time.hip)
    const int64_t *ring;           // [RB][N][3]
    void *signal;                  // gnuais_frame_signal[frame_cap], by ring slot
    int RB, N;
    int len;                       // rows of the call (<= 0: bits without samples)
    int64_t n0;                    // rows the chain had taken before it
    uint32_t pllinc;
    int n_taps, afc_window;
    int64_t v0;                    // first row of the current run of I/Q-type calls
};
hipError_t launch_frame_signal(const FrameSignalLaunch &a, hipStream_t stream);

// ---- the channel load per receiver (occupancy.hip; definition in include/gnuais_hip.h) ----
// launch_occ_code: behind launch_iq_power of the same call, on its stream.  codes[(j % CB) * N + c] = code(P_j) for the
// blocks j in [j0, j0 + count), which that call completed; sums is launch_iq_power's ring.  count <= RB and <= CB.
hipError_t launch_occ_code(const int64_t *sums, int RB, uint16_t *codes, int CB, int N, long long j0, int count,
                           hipStream_t stream);
// launch_occ_cover: behind the frame_signal launch of the same call, on its stream.  cover[(j % CB) * N + c] = 1 for the
// blocks j >= b0 of the cover span of every record with n0 <= times[i] < n0 + len.
struct OccCoverLaunch {
    const void *frames;            // gnuais_frame[frame_cap]: the ring K3 appended to
    const uint32_t *frame_count;
    uint32_t frame_cap;
    const int64_t *times;          // [frame_cap], by ring slot
    uint8_t *cover;                // [CB][N]
    int CB, N;
    int len;
    int64_t n0;
    uint32_t pllinc;
    int n_taps, afc_window;
    int64_t v0, b0;                // the run's first row and its first whole block
};
hipError_t launch_occ_cover(const OccCoverLaunch &a, hipStream_t stream);
// launch_occ_epoch: the finaliser of the epoch of E blocks from block `first` on, behind the cover launch of the call that
// made it final.  Writes the record of every channel to out[N], the tap word (code | busy << 14 | cover << 15) back into
// codes, the busy bit of the epoch's last block to carry[N] (read as the bit in front of the epoch unless first_epoch),
// and clears the epoch's cover bytes.  64 <= E <= 4096 < CB, 1 <= margin <= 255.
struct OccEpochLaunch {
    uint16_t *codes;               // [CB][N]
    uint8_t *cover;                // [CB][N]
    uint8_t *carry;                // [N]
    void *out;                     // gnuais_occupancy[N]
    int CB, N, E, margin;
    int64_t first;
    bool first_epoch;
};
hipError_t launch_occ_epoch(const OccEpochLaunch &a, hipStream_t stream);

// ---- utilities (util.hip) ---------------------------------------------------
hipError_t launch_tile_channels(const int16_t *base, int n_base, int len, int16_t *out,
                                int n_channels, hipStream_t stream);
hipError_t launch_crc16(const uint8_t *data, int stride, const int32_t *len, int n,
                        uint16_t *crc, hipStream_t stream);
// one frame's bits (a byte per bit) -> CRC + the bits byte-wise most-significant-first (util.hip)
hipError_t launch_crc16_bits(const uint8_t *bits, int n_bytes, uint16_t *crc, uint8_t *msb, int n_out,
                             hipStream_t stream);

// ---- complex baseband in: the FM discriminator (iq_disc.hip) ----------------------
// iq [len][N][2] int16 (I, Q) -> out [len][N] int16, the definition in include/gnuais_hip.h; carry [N][2] int16 is the
// previous pair of each channel, read at the start and replaced by row len-1.  iq and out must not overlap.
constexpr int IQ_DISC_ROWS = 64;     // rows per thread (a segment); each segment reads one row more
hipError_t launch_iq_discriminator(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, hipStream_t stream);

// ---- the carrier-error stage behind the discriminator (AFC: afc.hip, definition in include/gnuais_hip.h) ----
// n0 = rows the stage has taken before this call.  Three launches on one stream, in this order:
//   launch_iq_discriminator_afc  the discriminator, which also sums r and i over the blocks of AFC_BLOCK rows of n into
//                                blk [nb][N][2] int64 (block j in slot j % nb; nb >= W/64 + max_len/64 + 2);
//   launch_afc_estimate          e_j from the window sums, for the n_est blocks from j_lo on, into est [n_est][N];
//   launch_afc_apply             out[n] = a[n - W/2] - e, a from delay [W/2][N] (a[m] in row m % (W/2)) or from `audio`,
//                                est row 0 = block j_lo; then the call's last W/2 audio rows go into delay.
constexpr int AFC_BLOCK = 64;
constexpr int AFC_MIN_WINDOW = 128, AFC_MAX_WINDOW = 16384;
hipError_t launch_iq_discriminator_afc(const int16_t *iq, int16_t *out, int16_t *carry, int N, int len, int64_t *blk,
                                       int nb, unsigned long long n0, hipStream_t stream);
hipError_t launch_afc_estimate(const int64_t *blk, int nb, int N, int16_t *est, long long j_lo, int n_est, int W,
                               hipStream_t stream);
hipError_t launch_afc_apply(const int16_t *audio, int16_t *delay, const int16_t *est, long long j_lo, int16_t *out, int N,
                            int len, int W, unsigned long long n0, hipStream_t stream);

// ---- wideband in: the wide stage (wide_launch.hip over wide_kernels.h; host planning in resample_plan.h) ----
// in [len][M] pairs of sample format fmt (GNUAIS_FMT_*, wide_format.h) -> out [len*U/D][M*K][2] int16, len a multiple
// of D, the definitions in include/gnuais_hip.h (gnuais_batch_channeliser: U = 1; gnuais_batch_resampler).  hist [H][M]
// words is the carry (the last H = ceil((T-1)/U) wide samples, converted to int16 pairs), read here; the launch writes
// the next one into hist_out (another buffer).
constexpr int CHAN_MAX_K = 32;       // offsets per stream
struct WideLaunch {
    const void *in;        // [len][M] pairs in the launch's format; as int16: (I lo, Q hi)
    uint32_t *out;         // [len*U/D][M*K]
    const uint32_t *hist;  // [H][M]
    const uint32_t *mix;   // mixer tables, (C lo, S hi), offset k's at mix + off[k], per[k] entries
    const uint32_t *poly;  // fast form: the tap pairs, ResamplePlan::pairs at NA accumulators
    const int16_t *taps;   // direct form: [T]
    int M, K, D, T, len;
    int NA;                // fast form's accumulators per offset (channeliser_fast_na / resampler_fast_na), 0 = direct form
    int n_groups, seg_rows;                // set by launch_wide
    int per[CHAN_MAX_K], off[CHAN_MAX_K];
    int ph0[CHAN_MAX_K];   // (n mod per[k]) of the call's first wide sample
    const int32_t *groups; // fast form at a rational ratio: [U][3] = ResampGroup; null: the integer form (U = 1, groups of D)
    int U, H;              // H = T - 1 at U = 1
};
hipError_t launch_wide(const WideLaunch &a, int fmt, uint32_t *hist_out, hipStream_t stream);
// The launches of format F's kernels (wide_kernels.h), each defined once in the build, by the unit that holds those
// kernels: the integer fast form and the direct and carry kernels of int16 input in channeliser.hip, those of the other
// formats in channeliser_fmt.hip, the rational fast form of every format in resampler.hip.
template <int F, bool RATIONAL> hipError_t wide_fast_launch(const WideLaunch &a, dim3 grid, hipStream_t stream);
template <int F> void wide_direct_launch(const WideLaunch &a, dim3 grid, hipStream_t stream);
template <int F> void wide_carry_launch(const WideLaunch &a, uint32_t *hist_out, hipStream_t stream);

// ---- f1 on the device (nmea_device.hip) ---------------------------------------
size_t nmea_scratch_bytes(int n_frames, int n_chunks = 0);
// frames: device gnuais_frame[n]; seq_in/seq_out: device u8[n_channels] (seq_out preloaded with
// seq_in); out: device text buffer.  h_info: [0] bytes written, [1] sentences, [2] != 0 if a
// frame named a channel >= n_channels.  Synchronises `s`.
// frames[n] (device) -> out[n] (device) in print order: channel, then end_bit
hipError_t frames_sort(const struct gnuais_frame *frames, int n, struct gnuais_frame *out, void *scratch,
                       size_t scratch_bytes, hipStream_t s);
// the same, and times[n] (by ring slot, frame_time.hip) -> times_out[n] through the same permutation; words: a second
// array of 64-bit words by ring slot (the 8-byte records of frame_signal.hip), -> words_out[n] likewise
hipError_t frames_sort_timed(const struct gnuais_frame *frames, const int64_t *times, int n, struct gnuais_frame *out,
                             int64_t *times_out, void *scratch, size_t scratch_bytes, hipStream_t s,
                             const int64_t *words = nullptr, int64_t *words_out = nullptr);
// the device part only, queued without waiting; h_info4 (host, pinned): [0] + [1] bytes written,
// [2] sentences, [3] != 0 if a frame named a channel >= n_channels -- valid once `s` has got there
// n > 0: count known to the host, order by radix sort.  n < 0: the ring holds exactly one call; order and
// count (<= n_max) come from K3's chunk table (HdlcLaunch::chunks), nothing is read back.  *totals_dev:
// the device words h_info4 is copied from (h_info4 may be null).
hipError_t nmea_format_enqueue(const struct gnuais_frame *frames, int n, int n_max, int n_channels,
                               const uint8_t *seq_in, uint8_t *seq_out, char *out, size_t out_cap, void *scratch,
                               size_t scratch_bytes, uint32_t *h_info4, const uint2 *chunks, int n_chunks,
                               int chunk_passes, uint32_t **totals_dev, hipStream_t s);
// info8 (device): the formatter's four words (totals; null: nothing was formatted) + the ring's four counters
hipError_t nmea_slot_info_enqueue(const uint32_t *totals, const uint32_t *ring_count, uint32_t *info8_dev, hipStream_t s);
// device text -> pinned host text, length taken from info8 on the device; the info words follow it to the host
hipError_t nmea_text_copy_enqueue(const char *src, const uint32_t *info8_dev, char *dst_pinned, size_t dst_cap,
                                  uint32_t *info8_pinned, int workgroups, hipStream_t s);
// the stdout lines of protodec_getdata() for the same frames, right after nmea_format_enqueue(n > 0) on the same
// scratch and stream; lines: n * messages_line_bytes(), len / off: n words; info2 (device): [0] bytes, [1] lines
size_t messages_line_bytes();
hipError_t messages_format_enqueue(const struct gnuais_frame *frames, int n, int n_channels, const uint8_t *seq_in,
                                   const char *chanid_dev, void *scratch, size_t scratch_bytes, char *lines,
                                   uint32_t *len, uint32_t *off, char *out, size_t out_cap, uint32_t *info2,
                                   hipStream_t s);
// the batch's vessel table (gnuais_vessel per MMSI, sorted) folded on the device from the ring's frames
hipError_t vessels_fold_enqueue(const struct gnuais_frame *frames, int n, void *scratch, size_t scratch_bytes,
                                struct gnuais_vessel *out, int cap, uint32_t *count_dev, hipStream_t s);
// the vessel table carried on the device from batch to batch (one allocation of vessel_table_bytes(slots), zeroed;
// slots a power of two)
size_t vessel_table_bytes(uint32_t slots);
hipError_t vessel_table_update_enqueue(const struct gnuais_frame *frames, const uint32_t *count, int n_max, void *table,
                                       uint32_t slots, uint32_t *fslot, hipStream_t s);
hipError_t vessel_table_fetch(const void *table, uint32_t slots, struct gnuais_vessel *h_out, int max, int *n_out,
                              uint32_t h_info[4], hipStream_t s);
hipError_t nmea_format(const struct gnuais_frame *frames, int n, int n_channels, const uint8_t *seq_in,
                       uint8_t *seq_out, char *out, size_t out_cap, void *scratch, size_t scratch_bytes,
                       uint32_t *h_info, hipStream_t s);

// ---- repair of the candidates K3 counted in lostframes (hdlc_repair.hip; definition in include/gnuais_hip.h) ----
// One launch behind that call's K3, on its stream, in front of the frame_time launch and before the call's hand-off set
// (cand_first, cand_count) and the candidate slots can be reused.  Appends the repaired frames to the ring through
// frame_count[0] (overflow: frame_count[1]) and counts them in repaired[channel].
struct RepairLaunch {
    const uint32_t *cand;          // as in HdlcLaunch, of the K3 launch it follows
    const uint32_t *cand_first;
    const uint32_t *cand_count;
    int32_t *repaired;             // [N]
    void *frames;                  // gnuais_frame[frame_cap]
    uint32_t *frame_count;
    uint32_t frame_cap;
    int N, K;
};
hipError_t launch_hdlc_repair(const RepairLaunch &a, hipStream_t stream);

// ---- the long-frame deframer D': messages of three to five slots (hdlc_long.hip; definition in include/gnuais_hip.h) ----
// One launch behind the call's K3, on its stream, in front of the event that frees the call's hand-off set (segbits,
// segcnt) and before the next deframer launch moves ctl on.  D' walks the call's packs with a machine of its own (lctl),
// keeps the raw bits of the frame it is in in the channel's open record, and appends every frame of more than
// LONG_SHORT_BITS bits whose CRC holds to the long ring through frame_count[0] (overflow: frame_count[1]).
constexpr int LONG_CTL_WORDS = 3;        // [0] the machine's fields, [1] the open record's partial word, [2] its raw bits
constexpr int LONG_REC_WORDS = 40;       // the open record: 1030 stored bits + at most 206 stuffed zeros = 1236 raw bits
constexpr int LONG_FRAME_WORDS = 38;     // sizeof(gnuais_long_frame) / 4
constexpr int LONG_LIMIT_BITS = 1031;    // D' gives a frame up at this many stored bits: 1008 + 22 + 1
constexpr int LONG_SHORT_BITS = 426;     // a frame of at most this many bits is the chain's decoder's
struct LongLaunch {
    const uint32_t *segbits;       // as in HdlcLaunch, of the call's hand-off set
    const uint32_t *segcnt;
    const uint32_t *ctl;           // the chain's deframer's control state AFTER the call ([2], [5]: bits fed since reset)
    uint32_t *lctl;                // [LONG_CTL_WORDS][N]
    uint32_t *open;                // [LONG_REC_WORDS][N]
    int32_t *counters;             // [2][N]: long frames delivered, long frames that failed the CRC
    void *frames;                  // gnuais_long_frame[frame_cap]
    uint32_t *frame_count;         // [2]: frames appended, overflow flag
    uint32_t frame_cap;
    int N, n_seg, seg_words;
    int len;                       // rows of the call (<= 0: bits without samples, t = -1)
    int64_t n0;                    // rows the chain had taken before it
    // the repair of long frames (below): all null / 0 while it is off, and the launch is then the kernel without it
    uint32_t *clean = nullptr;     // [LONG_REC_WORDS][N]: where a closing frame is unstuffed, so that `open` stays raw
    uint32_t *cand = nullptr;      // [cand_cap][LONG_CAND_WORDS]: the call's candidate ring
    uint32_t *cand_count = nullptr;    // [2]: [parity] this call's count (zero at the launch), the other the next call's, cleared here
    uint32_t cand_cap = 0;
    int parity = 0;
};
hipError_t launch_hdlc_long(const LongLaunch &a, hipStream_t stream);
// protodec_reset() for D' (counters: also its three counters [3][N] -- delivered, failed, repaired -- else null)
hipError_t launch_hdlc_long_reset(uint32_t *lctl, int32_t *counters, int N, hipStream_t stream);

// ---- repair of the long frames D' counted in `failed` (hdlc_long_repair.hip; definition in include/gnuais_hip.h) ----
// One launch behind D''s of the same call, on its stream.  D' (in its form that keeps the raw bits) appended one record
// per failed frame to the candidate ring; this launch reads the count D' left, tries every pair flip of every record
// (the trial is hdlc_repair.h's with LongLimits) and appends the frames with exactly one passing trial to the long ring
// through frame_count[0] (overflow: frame_count[1]), counting them in repaired[channel].
// A candidate record: [0] channel, [1] stamp bits 31:0, [2] [3] t, [4] n | stamp bits 36:32 << 16, [5] rawlen, then the
// LONG_REC_WORDS raw words (zero behind rawlen).
constexpr int LONG_CAND_HDR = 6;
constexpr int LONG_CAND_WORDS = LONG_CAND_HDR + LONG_REC_WORDS;
struct LongRepairLaunch {
    const uint32_t *cand;          // as in LongLaunch, of the D' launch it follows
    const uint32_t *cand_count;    // the word that launch counted in: its cand_count + parity
    uint32_t cand_cap;
    int32_t *repaired;             // [N]
    void *frames;                  // gnuais_long_frame[frame_cap]
    uint32_t *frame_count;
    uint32_t frame_cap;
    int N;
    int blocks;                    // the fixed grid: workgroups of one wave, candidate i is taken by workgroup i mod blocks
};
hipError_t launch_hdlc_long_repair(const LongRepairLaunch &a, hipStream_t stream);

// ---- the signal record of every long frame (long_signal.hip; gnuais_batch_long_frame_signal in include/gnuais_hip.h) ----
// One launch behind D''s (and the long repair's) of the same call, on its stream.  Writes signal[i] for every record i of
// the long ring with t < 0 -- (0, 0, 0) -- or n0 <= t < n0 + len; other records are left alone.  With `cover` it also
// stores 1 into the cover ring for the blocks j >= b0 of the cover span of every record with n0 <= t < n0 + len
// (launch_occ_cover's rule, with the run's first row occ_v0).
struct LongSignalLaunch {
    const void *frames;            // gnuais_long_frame[frame_cap]: the long ring
    const uint32_t *frame_count;   // its two words ([0] = records appended)
    uint32_t frame_cap;
    const int64_t *ring;           // [RB][N][3]: launch_iq_power's ring
    void *signal;                  // gnuais_frame_signal[frame_cap], by ring slot
    int RB, N;
    int len;                       // rows of the call (<= 0: bits without samples)
    int64_t n0;                    // rows the chain had taken before it
    uint32_t pllinc;
    int n_taps, afc_window;
    int64_t v0;                    // first row of the current run of I/Q-type calls
    uint8_t *cover = nullptr;      // [CB][N], or null: no cover bytes
    int CB = 0;
    int64_t occ_v0 = 0, b0 = 0;    // the run the epochs are counted in: its first row and its first whole block
};
hipError_t launch_long_signal(const LongSignalLaunch &a, hipStream_t stream);

// ---- one record per transmission: the duplicate merge of a drain, for the short and the long frames (frame_unique.hip;
// gnuais_batch_unique and gnuais_batch_long_unique in include/gnuais_hip.h) ----
// Entries = [tail | ring]: n_tail open clusters of earlier drains and the `have` frames of the ring.  Short kind: a tail
// entry is 16 words (t_last, then the key as a record holds it), the frames' times lie beside the ring, every buffer is
// 16-byte aligned.  Long kind: a tail entry is a 38-word record with t_last in its t words and word 4 masked to the key,
// the member time is the record's own t (times and out_times stay null), every buffer is 8-byte aligned, and the signal
// records are long_signal.hip's, where it is on.
// unique_cluster_enqueue() queues everything up to the compacted primaries and the next tail (tail_out: room for
// n_tail + have entries, another buffer than tail) and leaves UNIQUE_INFO_WORDS words at unique_info(scratch); `exact`:
// group by the key words themselves instead of the hash -- what the caller repeats the call with when the collision word
// came back set (nothing of the first attempt is kept).  unique_deliver_enqueue() then sorts the n_primaries into output
// order and gathers out_frames / out_times / out_copies.
constexpr int UNIQUE_INFO_COLLISION = 0;    // != 0: equal hashes with unequal keys were seen
constexpr int UNIQUE_INFO_CLUSTERS = 1;
constexpr int UNIQUE_INFO_PRIMARIES = 2;    // records to deliver
constexpr int UNIQUE_INFO_TAIL = 3;         // entries written to tail_out
constexpr int UNIQUE_INFO_LATE = 4;         // two words: late copies of this drain (uint64)
constexpr int UNIQUE_INFO_WORDS = 8;
enum class UniqueKind { Short, Long };      // gnuais_frame (the default wherever a kind is taken) / gnuais_long_frame
struct UniqueLaunch {
    UniqueKind kind = UniqueKind::Short;
    const void *frames;            // gnuais_frame[have] / gnuais_long_frame[have]: the ring
    const int64_t *times = nullptr;     // short: [have], by ring slot
    int have;
    const void *tail;              // [n_tail][16] / [n_tail][38] words
    int n_tail;
    void *tail_out;
    long long window, rows;        // W, and the batch's row count at the drain
    int hash_bits;                 // 1..64: bits of the hash in use (set_option("unique_hash_bits"))
    int ch_bits, time_bits;        // channel < 2^ch_bits, t + 1 < 2^time_bits: the width of the member-order word
    void *scratch;
    size_t scratch_bytes;          // >= unique_scratch_bytes(n_tail + have, kind)
    void *out_frames;              // records of the kind
    int64_t *out_times = nullptr;  // short
    int32_t *out_copies;
    // the member lists (gnuais_batch_drain_frames_heard, _long_frames_heard); out_first null: no lists wanted, and the
    // rest is not read.  unique_deliver_enqueue() then also fills out_first[n_primaries + 1] (the running sum of
    // out_copies, from 0) and out_members[sum of the copies <= have] (16-byte aligned for the short kind, 8-byte for the
    // long), from the records, times and `signal` by ring slot.
    const void *signal = nullptr;               // gnuais_frame_signal[have], or null: zeros
    void *heard_scratch = nullptr;
    size_t heard_scratch_bytes = 0;             // >= unique_heard_scratch_bytes(have)
    int32_t *out_first = nullptr;
    struct gnuais_hearer *out_members = nullptr;
};
size_t unique_scratch_bytes(int n_entries, UniqueKind kind = UniqueKind::Short);
size_t unique_heard_scratch_bytes(int have);
uint32_t *unique_info(void *scratch);
hipError_t unique_cluster_enqueue(const UniqueLaunch &a, bool exact, hipStream_t s);
hipError_t unique_deliver_enqueue(const UniqueLaunch &a, int n_primaries, hipStream_t s);

} // namespace gnuais
