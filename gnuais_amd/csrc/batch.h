// batch.h -- what the three host units of the C ABI share (gnuais_capi.hip, capi_ingest.hip, capi_delivery.hip): the
// owners of a batch's device resources, struct gnuais_batch, the error helpers and the few functions that more than
// one unit calls.  Internal to csrc; not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gnuais_hip.h"
#include "kernels.h"

using namespace gnuais;

namespace gnuais {
// Sets gnuais_last_error() to `what` (and HIP's text for e) and returns code
int fail(int code, const char *what, hipError_t e = hipSuccess);
}

#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) return fail(GNUAIS_E_HIP, #expr, e_);            \
    } while (0)

namespace gnuais {
// The owners of what a batch holds.  Each releases its resource exactly once -- when it is told to, when it is given
// another, or when the batch is deleted (gnuais_batch_destroy has made the batch's device current by then) -- so a
// half-built batch and a batch that used every feature end the same way, without a list.  Move-only.  Nothing more:
// no sharing, no pooling; the aliases in gnuais_batch (s_k, s_post, s_copy, e_in_hook) stay plain handles.

// Device memory (PINNED: page-locked host memory) and its size in bytes
template <class T, bool PINNED = false>
struct Buf {
    T *p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~Buf() { (void) release(); }
    operator T *() const { return p; }
    hipError_t release()
    {
        const hipError_t e = !p ? hipSuccess : PINNED ? hipHostFree(p) : hipFree(p);
        p = nullptr;
        bytes = 0;
        return e;
    }
    // n bytes anew (zeroed: device memory cleared); empty with size 0 on failure
    hipError_t alloc(size_t n, bool zeroed = false)
    {
        hipError_t e = release();
        if (e == hipSuccess) e = PINNED ? hipHostMalloc((void **) &p, n, hipHostMallocDefault) : hipMalloc((void **) &p, n);
        if (e != hipSuccess) return p = nullptr, e;
        bytes = n;
        if (zeroed) e = PINNED ? (memset(p, 0, n), hipSuccess) : hipMemset(p, 0, n);
        if (e != hipSuccess) (void) release();
        return e;
    }
    // allocated on first use: nothing happens when it exists (also what an attempt that failed further on left behind)
    hipError_t ensure(size_t n, bool zeroed = false) { return p ? hipSuccess : alloc(n, zeroed); }
    // scratch that grows on demand: when `need` exceeds what it holds, it is freed and allocated anew with `need + slack`
    hipError_t grow(size_t need, size_t slack = 0) { return bytes >= need ? hipSuccess : alloc(need + slack); }
};
template <class T> using Pinned = Buf<T, true>;

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void) hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    // created only if it does not exist yet
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

// a non-blocking stream
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    // created only if it does not exist yet (priority 0: the default one)
    hipError_t ensure(int priority = 0) { return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
};

} // namespace gnuais

namespace gnuais {
// The wide stage in front of the discriminator (wide_kernels.h): out rate = in rate * U / D, U = 1 for
// gnuais_batch_channeliser.  The configuration, the device tables, the carry (the last H = ceil((T-1)/U) wide samples of
// each stream, double-buffered: a launch reads hist[cur] and writes the other) and the wide-sample count n.
struct WideStage {
    int K = 0, U = 1, D = 0, T = 0, H = 0, R = 0, NA = 0;   // K == 0: not configured; NA: the fast form's accumulators, 0 = direct
    int per[CHAN_MAX_K] = {}, off[CHAN_MAX_K] = {};
    Buf<uint32_t> mix, poly, hist[2];
    Buf<int32_t> groups;            // the fast form's group table at a rational ratio; none: the integer form's kernels
    Buf<int16_t> taps;
    int cur = 0;
    unsigned long long n = 0;
};
} // namespace gnuais

// The stages a call may pass through, in launch order: the channeliser, the discriminator, the carrier-error stage
// (gnuais_batch_afc, when it is on), the chain (K1 .. K3)
enum Stage { CHAN, DISC, AFC, CHAIN, N_STAGES };

// The input forms (include/gnuais_hip.h): audio [len][N], I/Q [len][N][2], wideband [len][N/K][2]
enum FormId { AUDIO, IQ, WIDE };

struct gnuais_batch {
    int device = 0;
    int N = 0, NT = 0, NE = 0, d = 0;
    uint32_t pllinc = 0;
    int max_len = 0, frame_cap = 0;
    int sgn_words = 0, bits_words = 0;
    std::vector<float> taps;
    float te[128] = {0};
    // device state
    // The FIR's carry (the last NT input rows) and the per-call peak buffers rotate over HB buffers: call i reads
    // hist[i % HB], writes hist[(i + 1) % HB], gathers its peaks in maxval[i % HB] and clears maxval[(i + 2) % HB].
    // (Two would do for FIR launches that run one after the other; four keep the writer of a buffer two calls away
    // from its readers.)
    static constexpr int HB = 4;
    Buf<int16_t> hist[HB];
    int hist_cur = 0;
    // every hand-off buffer exists NBUF times; `nbuf` of them are in use (index = call % nbuf), so K1 can run up
    // to nbuf-1 calls ahead of the sequential stages
    static constexpr int NBUF = 8;
    // Depth in use.  The host waits for K3 of call i-nbuf before it launches the FIR of call i, so the pipeline is a
    // closed loop: period >= latency of a call / nbuf.  Round 4, C3, same box (profiles/r04_nbuf_3_vs_4.txt): depth 3
    // and 4 give the same steady state (0.518 ms: at 3 the loop's bound and the PLL stage's duration meet), 5-8 no
    // better (0.53-0.55), 2 starves (0.70); a short timed region ends sooner with fewer calls in flight to drain
    // (20 steps: 0.574 against 0.583), so 3.
    int nbuf = 3;
    int sets_alloc = 0;                         // hand-off sets that exist (>= nbuf)
    Buf<uint32_t> sgn[NBUF];                    // K1 -> K2
    Buf<uint32_t> pll, lastbit, prev;           // receiver.h:38-44, carried by K2
    int n_cu = 256;
    Buf<uint32_t> segbits[NBUF];                // K2 -> K2b
    Buf<uint32_t> segcnt[NBUF];
    int n_seg = 0, seg_words = 0;
    // stage pipeline: K1 on the caller's stream and one internal stream per later
    // kernel, so that the short-on-parallelism stages of call i overlap the FIR of
    // call i+1 (and each other).
    hipStream_t s_k[4] = {nullptr, nullptr, nullptr, nullptr};   // K2, (spare), K2b, K3 (entries of pool[])
    hipStream_t s_k_default[4] = {nullptr, nullptr, nullptr, nullptr};
    static constexpr int POOL = 12;
    Stream pool[POOL];                          // candidates for gnuais_batch_autotune(): [0..3] the default
                                                // assignment, [0..7] high priority, [8..11] default priority
    Event e_done[5][NBUF];                      // e_done[s][k]: stage s of the call using set k is done
                                                // (0 K1, 1 K2, 3 K2b, 4 K3)
    unsigned long long calls = 0, hdlc_calls = 0;   // run calls / K3 launches since the last drain
    bool pipeline = true;
    Buf<uint32_t> ctl, cand;
    Buf<uint32_t> cand_first[NBUF], cand_count[NBUF];   // K2b -> K3
    int cand_K = 64;
    Buf<int32_t> counters;
    Buf<int> maxval[HB];                   // rotate with the history buffers
    int max_cur = 0, max_last = 0;
    Buf<float> d_taps;
    Buf<MfmaTaps> d_mfma;           // fir_sign_mfma.hip: the 48 central taps as integer Toeplitz operands (long tables)
    // f1 on the device (gnuais_batch_drain_nmea): allocated on first use
    Buf<uint8_t> d_seq[2];
    Buf<char> d_text;
    Buf<void> nmea_scratch;
    Buf<char> d_msg;                // gnuais_batch_drain_messages: lines, lengths, offsets, packed text
    Buf<uint32_t> d_word;           // a few device words for counts read back by the drain-type calls
    // the vessel table carried on the device (gnuais_batch_vessel_table_*): one allocation, per-frame slot scratch
    Buf<void> vt;
    Buf<uint32_t> vt_fslot;
    uint32_t vt_slots = 0;
    int vt_capacity = 0;
    // The frame ring K3 appends to and its four counters: ring[ring_cur] / ring_count[ring_cur].  Ring 0 exists from
    // create on and is the only one a batch that does not stream ever uses; gnuais_batch_stream_nmea makes the
    // other NRING - 1 on its first call.  A ring is filled by K3; its formatter and the copy of its
    // text into pinned memory are queued behind that K3 at once, with every size taken on the device; the
    // text is handed out NRING - 1 calls later, which is the only thing the host ever waits for.  A call
    // is about 2.7 ms from its FIR to its text on the host (four chain stages, formatter, PCIe copy), so
    // about six of them have to be in flight for one to finish every 0.55 ms.
    static constexpr int NRING = 8;
    Buf<gnuais_frame> ring[NRING];
    Buf<uint32_t> ring_count[NRING];
    Buf<uint2> ring_chunks[NRING];              // K3's chunk table per ring (kernels.h: HdlcLaunch::chunks)
    int ring_runs[NRING] = {};                  // K3 launches into the ring since it became current
    int n_chunks = 0;
    // gnuais_batch_discard_frames leaves no dispatch behind: it sets discard_pending, and the next deframer launch empties
    // ring 0's words itself (HdlcLaunch::discard), behind the last K3 and in front of its own in stream order.  Whatever
    // reads or hands out ring 0 or its words before that launch -- the drains, the counts, reset, the switch to
    // streaming, a call without a deframer -- calls discard_flush() first, which issues the memset the discard used to be.
    // discard_launches counts the launches that carried the flag (the parity of HdlcLaunch::ovf_mark).
    bool discard_pending = false;
    hipStream_t discard_stream = nullptr;       // the stream the last discard named (the chain's, when it is not pipelined)
    unsigned discard_launches = 0;
    // Experiments (GNUAIS_CYCLE, bits): 1 = the discard rides on the deframer launch (else: a memset per discard, as
    // before), 2 = no event record between the deframer and a K3 on the same stream.  Default 3.
    int cycle_parts = 3;
    // The receive time of every frame (gnuais_batch_frame_times, frame_time.hip; off by default).  `rows` counts the rows
    // the chain has taken since create / reset, over every kind of run call, whether the feature is on or not; while it
    // is on, one more launch behind each K3 writes times[slot] for the records that K3 appended to ring 0 (a batch with
    // the feature on does not stream).  The kernel finds its records by their end_bit, so there is no state here that
    // the drains, discard_frames or the resets would have to clear.
    bool frame_times = false;
    unsigned long long rows = 0;
    bool clock_fresh = true;                    // no run or decode call since create / reset: gnuais_batch_set_clock may move the clocks
    Buf<int64_t> times;                         // [frame_cap], allocated when the feature is first switched on
    // The signal power and carrier error of every frame (gnuais_batch_frame_signal, frame_signal.hip; off by default;
    // needs frame_times).  While it is on, every I/Q-type call launches the ingest kernel in front of its discriminator
    // (block sums of P, r, i into fs_ring) and every K3 gets one more launch behind its frame_time launch, which
    // writes signal[slot].  fs_v0: first row of the current run of I/Q-type calls; fs_end: the row behind the last
    // I/Q-type call (rows != fs_end at the next one: an audio-type call came between, a new run starts); fs_iq_call:
    // the run call under way came through run_form, so its rows are I/Q rows (else its frames get (0, 0, 0)).
    bool frame_signal = false, fs_iq_call = false;
    int fs_RB = 0, fs_nbuf = 0;                 // slots of the ring; the nbuf it was sized for
    unsigned long long fs_v0 = 0, fs_end = 0;
    Buf<int64_t> fs_ring;                       // [fs_RB][N][3] (P, R, I), block j of n in slot j % fs_RB
    Buf<uint32_t> fs_carry;                     // [N] the stage's own previous pair
    Buf<gnuais_frame_signal> signal;            // [frame_cap], parallel to times
    // The channel load per receiver (gnuais_batch_occupancy, occupancy.hip; occ_E = 0: off; needs frame_signal).  While it
    // is on, every I/Q-type call launches the code kernel behind its ingest kernel and the cover kernel behind its
    // frame_signal launch, and the call that makes an epoch final launches the finaliser behind that.  occ_v0: the first
    // row of the run the epochs are counted in (fs_v0, or the row the feature was switched on at when that is later);
    // occ_next: the run's epochs that are final; occ_seq: final epochs since switch-on / reset, epoch s in slot s % 64 of
    // occ_out with its first block in occ_first; occ_drained: the next one a drain delivers.
    int occ_E = 0, occ_margin = 0, occ_CB = 0, occ_nbuf = 0, occ_W = 0;     // occ_nbuf, occ_W: the depth and the AFC window the rings are sized for
    bool occ_cover_clean = false;               // the cover ring is all zero: the start of a run has nothing to clear
    unsigned long long occ_v0 = 0, occ_seq = 0, occ_drained = 0;
    long long occ_next = 0, occ_lost = 0;
    long long occ_first[64] = {};
    Buf<uint16_t> occ_codes;                    // [occ_CB][N], block j of n in slot j % occ_CB
    Buf<uint8_t> occ_cover, occ_carry;          // [occ_CB][N]; [N] the busy bit of the last final epoch's last block
    Buf<gnuais_occupancy> occ_out;              // [64][N]
    // The repair of CRC-failed candidates (gnuais_batch_repair, hdlc_repair.hip; off by default): while it is on, one
    // more launch behind each K3 -- in front of the frame_time launch -- appends the repaired frames to ring 0 (a batch
    // with the feature on does not stream) and counts them per channel.
    bool repair = false;
    Buf<int32_t> repaired;                      // [N], allocated (zeroed) when the feature is first switched on
    // Messages of three to five slots (gnuais_batch_long_frames, hdlc_long.hip; off by default): while it is on, one more
    // launch behind each K3 runs the second decoder D' over the call's bit packs and appends its frames to a ring of its
    // own (a batch with the feature on does not stream).  Everything is allocated when the feature is first switched on:
    // D''s machine [LONG_CTL_WORDS][N], the open record [LONG_REC_WORDS][N], its counters [3][N] (delivered, failed,
    // repaired), the ring of long_cap records and its two words (frames appended, overflow flag).
    bool long_frames = false;
    int long_cap = 0;
    Buf<uint32_t> long_ctl, long_open, long_count;
    Buf<int32_t> long_counters;
    Buf<gnuais_long_frame> long_ring;
    // The repair of the long frames D' counts in `failed` (gnuais_batch_long_repair, hdlc_long_repair.hip; off by default,
    // only with long_frames): while it is on, D' runs in its form that keeps the raw bits -- it unstuffs a closing frame
    // into long_clean [LONG_REC_WORDS][N] and appends every failed one to the candidate ring long_cand
    // [long_cand_cap][LONG_CAND_WORDS] -- and one more launch behind it repairs what the ring holds.  The ring is sized
    // like the long ring (every close of one call fits) and consumed within the call.  long_cand_count holds two
    // counters used by call parity: D' of a call counts in [long_parity] and clears the other, which the repair launch
    // of the call before has read by then -- no memset command between the calls.  Allocated on first use.
    bool long_repair = false;
    int long_cand_cap = 0;
    int long_parity = 0;
    Buf<uint32_t> long_clean, long_cand, long_cand_count;
    // The signal record of every long frame and its share in the channel load (gnuais_batch_long_frame_signal,
    // long_signal.hip; off by default, only with long_frames and frame_signal): while it is on, one more launch behind D'
    // and the long repair writes long_signal[slot] for the call's records, and -- where gnuais_batch_occupancy was switched
    // on with it (occ_long: LAG and the rings are those of the 1008-bit span) -- their cover bytes, in front of the call's
    // epoch finalisers.  fs_long: the signal ring is sized for the long span (it stays so until frame_signal is switched).
    bool long_frame_signal = false, fs_long = false, occ_long = false;
    Buf<gnuais_frame_signal> long_signal;       // [long_cap], parallel to long_ring
    // One record per transmission (frame_unique.hip), a state per kind of frame: uq for gnuais_batch_unique, lq for
    // gnuais_batch_long_unique (only with long_frames).  Nothing runs per call; only the drains
    // gnuais_batch_drain_frames_unique / _heard and gnuais_batch_drain_long_frames_unique / _heard touch any of it.
    struct UniqueState {
        int window = 0;                         // in rows; 0 = off
        int cur = 0, n_tail = 0;                // the open clusters carried from drain to drain ([n][16] / [n][38] words),
        Buf<uint64_t> tail[2];                  // double-buffered: a drain reads tail[cur] and writes the other
        long long late = 0;                     // the late copies counted so far
        Buf<void> scratch;                      // the stage's scratch, which grows on first use like nmea_scratch
        Buf<void> heard;                        // the member lists' own scratch, on the first _heard drain
    };
    UniqueState uq, lq;
    int uq_hash_bits = 64;                      // the bits of the hash in use, for both (set_option("unique_hash_bits"))
    Buf<char> lq_out;                           // the long drain's output (records, copies, offsets, members), on demand
    // 0 whenever the batch is not streaming: only gnuais_batch_stream_nmea advances it, behind the point where it has
    // set `streaming`; set_option("streaming", 0), the one place that clears `streaming`, and reset set it to 0
    // (rings_reset)
    int ring_cur = 0;
    bool streaming = false;
    hipStream_t s_post = nullptr, s_copy = nullptr;     // s_copy: s_copy_own, or the pool stream autotune_delivery chose
    Stream s_copy_own;                          // the one created for the copy
    Event e_fill[NRING], e_fmt[NRING], e_txt[NRING];
    Buf<char> sd_text[NRING];                   // device text per slot
    Pinned<char> sh_text[NRING];                // pinned host text per slot
    Pinned<uint32_t> sh_info;                   // pinned: [NRING][8]: format's 4 words, the ring's 4 counters
    int s_stage[NRING] = {};                    // 1: the slot's formatter is queued, its text not handed out yet
    size_t sh_text_want = 0;                    // pinned text buffers grow to this (learnt from the traffic)
    Buf<uint32_t> sd_info;                      // device: [NRING][8], what sh_info receives with the text
    bool copy_on_k3 = false;                    // experiment: the copy kernel on K3's stream as well
    int copy_wgs = 24;                          // waves of the device -> pinned copy (measured: 16 0.65, 24 0.62, 32 0.64, 64 0.79 ms per C3 step)
    Buf<uint8_t> sd_seq[2];                     // per-channel sequence digit, carried on the device
    int sd_seq_cur = 0;
    unsigned long long stream_calls = 0;
    Buf<int16_t> stage_x;
    Buf<float> stage_f;             // gnuais_batch_filter_host: the floats on their way out
    // gnuais_batch_run_host_async: two pinned host buffers + two device buffers, one internal stream
    Pinned<int16_t> pin[2];
    Buf<int16_t> dev_in[2];
    size_t pin_bytes = 0;                       // the size of all four once they exist
    Stream s_io;
    Event e_in[2];                              // the FIR of the call that used staging pair q is done
    hipEvent_t e_in_hook = nullptr;             // run_host_async -> run: record this right behind K1
    unsigned long long host_calls = 0;
    // options
    FirOptions fir;                             // the fir_* options the choice of the FIR kernel depends on (fir_plan.h)
    SignBounds sign;                            // the sign-exact slicer's error bounds for the table (fir_plan.h)
    int stage_mask = 0x1f;                      // experiments only: bit s = launch stage s
    int k0 = 0;                     // first effective tap
    int pll_variant = 0;            // 0: by channel count; 7 / 8 (kernels.h: PllLaunch::variant)
    int hdlc_lpw = 0;               // channels per wave in K2b; 0 = the variant's own default (16 event-driven, 64 bit-serial)
    int hdlc_variant = 1;           // 1: the event-driven deframer (hdlc_events.hip), 0: window by window (hdlc_crc.hip)
    bool timing = false;
    int timing_stride = 1;          // time every n-th call only: ten event records a call are not free
    // timing: a ring of per-call event sets so that kernel durations can be read back
    // for every call of a timed region, not just the last one
    static constexpr int TIMING_RING = 64;
    Event evr[TIMING_RING][10];            // 0,1 K1 | 2,6 K2 | 5,7 K2b | 9,4 K3
    unsigned long long timed_calls = 0;
    int last_k = 0;
    bool timed_last = false;
    // The drain rule: each stage keeps the stream of its last launch here (last[CHAIN].s is also the stream that
    // gnuais_batch_sync drains).  Before a call launches anything on stream s, it drains the recorded stream of every
    // stage it passes through, when that stream is not s (drain()).  This covers two hazards.  A stage's carry goes
    // from launch to launch in stream order: the channeliser's history, the discriminator's previous pair, the chain's
    // FIR history and peaks.  And a stage in front of the chain overwrites an intermediate buffer whose reader is the
    // next stage of the previous call, on that call's stream: wide_iq is read by the discriminator, iq_audio by K1 or the
    // AFC stage, afc_audio by K1.  The AFC stage's delay line, block sums and estimates are carries of the first kind.
    struct { hipStream_t s = nullptr; bool used = false; } last[N_STAGES];
    int last_len = 0;
    int pll_form = 0;               // what pll_form_of() gave for the last run call's PLL launch: 7 / 8; 0 before any call
    // K3 on the deframer's stream: at ring lag 1 the two never overlap (deframer(i) -> K3(i) -> deframer(i+1)), so the two
    // cross-stream event waits per call in the loop that sets the period become stream order: 20-step 0.550 -> 0.544,
    // steady 0.527 -> 0.522 (three A/B pairs, profiles/r04_k3_on_the_deframers_stream.txt).  0 = a stream of its own.
    int k3_same = 1;
    // complex baseband in (gnuais_batch_run_iq / _discriminate, iq_disc.hip): the discriminator's carry -- the last (I, Q)
    // pair an I/Q call saw, per channel -- and the audio it writes for the chain, [max_len][N] (allocated on first use).
    Buf<int16_t> iq_prev;                       // [N][2]
    Buf<int16_t> iq_audio;
    // wideband in (gnuais_batch_channeliser / _resampler / _run_wideband): the wide stage, and the narrowband I/Q it
    // writes for the discriminator, [max_len][N][2] (allocated on first use)
    WideStage wide;
    Buf<int16_t> wide_iq;
    // the carrier-error stage (gnuais_batch_afc, afc.hip; 0 = off): the window W, the rows n it has taken, the ring of
    // block sums [afc_nb][N][2], the delay line [W/2][N], the estimates of the last call [max_len/64 + 2][N] with the row
    // that serves the last output row (-1: none yet), and the corrected audio it writes for the chain, [max_len][N]
    // (allocated on first use)
    int afc_W = 0, afc_nb = 0, afc_est_row = -1;
    unsigned long long afc_n = 0;
    Buf<int64_t> afc_blk;
    Buf<int16_t> afc_delay, afc_est, afc_audio;
};

// Per `up` chain rows, `rows` input rows of `cols` columns of `bytes` bytes each (up > 1: the rational channeliser);
// `stages`: bit s = the call passes stage s
struct Form {
    int bytes, cols, rows;
    unsigned stages;
    int up = 1;
    size_t bytes_of(int in_rows) const { return (size_t) bytes * (size_t) cols * (size_t) in_rows; }
};

namespace gnuais {
int set_device(const gnuais_batch *b);
// The drain rule (gnuais_batch::last): drains the recorded stream of each stage in `stages` that is not s
int drain(gnuais_batch *b, unsigned stages, hipStream_t s);
// the stream K3 runs on, and the stream behind the last K3 (when the chain runs on the caller's stream: that one)
hipStream_t k3_stream(const gnuais_batch *b);
hipStream_t behind_k3(const gnuais_batch *b);
// capi_delivery.hip: a pending discard (gnuais_batch::discard_pending) takes effect now, as a memset behind the last K3
int discard_flush(gnuais_batch *b);
// gnuais_capi.hip: the long ring's two words once the chain is idle, in the name of the entry `who`: records held, and
// whether some were dropped (GNUAIS_E_STATE on a batch that never decoded long frames)
int long_pending(gnuais_batch *b, const char *who, uint32_t &have, bool &overflow);
double now_ms();
// capi_ingest.hip: the carries of the stages in front of the chain, for gnuais_batch_reset
int chan_zero_state(gnuais_batch *b);
int afc_zero_state(gnuais_batch *b);
// capi_ingest.hip: gnuais_batch_occupancy's part of a reset (the device is idle), and of the tail of an I/Q-type call of
// len rows from row b->rows on, behind its frame_signal launch on stream s: the cover launch (occ_cover), and the
// finalisers of the epochs that call makes final (occ_finalise) -- directly behind it, or behind the long frames' cover
// where they have one (gnuais_batch_long_frame_signal; long_signal_launch fills that launch, cover bytes included)
int occ_zero_state(gnuais_batch *b);
int occ_cover(gnuais_batch *b, const HdlcLaunch &h, int len, hipStream_t s);
int occ_finalise(gnuais_batch *b, int len, hipStream_t s);
LongSignalLaunch long_signal_launch(const gnuais_batch *b, int len);
}
