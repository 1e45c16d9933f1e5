// gnuais_capi.hip -- host side of the C ABI declared in include/gnuais_hip.h.
//
// Owns the per-batch device state (FIR history, PLL phase, deframer state,
// frame ring) and sequences the kernels of one receiver_run() pass:
//   K1 fir_slice (+ history carry) -> K2 pll -> K2b hdlc_deframe -> K3 hdlc_crc
// K1 on the caller's stream, every later stage on an internal stream of its own, chained by
// events over four sets of hand-off buffers, so that the stages of consecutive calls overlap
// (DESIGN.md 4.6); `pipeline` = 0 runs them back to back on the caller's stream instead.
// No CPU implementation of the chain exists here: without a usable HIP device every entry
// point fails with GNUAIS_E_HIP.
// This unit: error state, create / destroy / reset / options, the chain, the stage entry points, read-outs, info,
// timing, the batch-less utilities.  The input forms in front of the chain are capi_ingest.hip, what becomes of the
// frames capi_delivery.hip; batch.h holds the batch and the owners of its device resources.
#include <chrono>

#include "batch.h"
#include "occupancy.h"

namespace gnuais {
namespace scalar { hipError_t launch_fir_slice(const FirLaunch &a, hipStream_t stream); }
}

static thread_local std::string g_err;

int gnuais::fail(int code, const char *what, hipError_t e)
{
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

// src/receiver.c:39-49, first half of the symmetric table (double literals that
// round to fp32 on assignment, exactly as the reference's static float array)
static const double k_tap_half[18] = {
    2.5959e-55, 2.9479e-49, 1.4741e-43, 3.2462e-38, 3.1480e-33, 1.3443e-28,
    2.5280e-24, 2.0934e-20, 7.6339e-17, 1.2259e-13, 8.6690e-11, 2.6996e-08,
    3.7020e-06, 2.2355e-04, 5.9448e-03, 6.9616e-02, 3.5899e-01, 8.1522e-01};

// The drain rule (gnuais_batch::last): drains the recorded stream of each stage in `stages` that is not s.  The
// stage's earlier launches are then done, so s stands for them from here on.
int gnuais::drain(gnuais_batch *b, unsigned stages, hipStream_t s)
{
    for (int q = 0; q < N_STAGES; ++q) {
        auto &l = b->last[q];
        if (!(stages >> q & 1u) || !l.used || l.s == s) continue;
        HIP_TRY(hipStreamSynchronize(l.s));
        l.s = s;
    }
    return GNUAIS_OK;
}

int gnuais::set_device(const gnuais_batch *b)
{
    HIP_TRY(hipSetDevice(b->device));
    return GNUAIS_OK;
}

double gnuais::now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the stream K3 runs on (and everything that has to come behind the last K3)
hipStream_t gnuais::k3_stream(const gnuais_batch *b)
{
    // not while the batch is streaming: K3 then waits for the delivery side (a frame ring to come free), and on the
    // deframer's stream that wait would hold the next deframer launch too (0.89 against 0.62 ms per delivered step)
    return (b->k3_same && !b->streaming) ? b->s_k[2] : b->s_k[3];
}

hipStream_t gnuais::behind_k3(const gnuais_batch *b) { return b->pipeline ? k3_stream(b) : b->last[CHAIN].s; }

// the state read-outs: once the chain is idle, n elements at d into v
template <class T>
static int read_out(gnuais_batch *b, const void *d, size_t n, std::vector<T> &v)
{
    if (int rc = gnuais_batch_sync(b)) return rc;
    v.resize(n);
    HIP_TRY(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

// the long ring's two words and what they say: records held, and whether some were dropped (capi_delivery.hip's merged
// drains read them too)
int gnuais::long_pending(gnuais_batch *b, const char *who, uint32_t &have, bool &overflow)
{
    if (!b->long_ctl) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: the batch has never decoded long frames (gnuais_batch_long_frames)", who);
        return fail(GNUAIS_E_STATE, msg);
    }
    if (int rc = gnuais_batch_sync(b)) return rc;
    uint32_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpy(cnt, b->long_count, sizeof cnt, hipMemcpyDeviceToHost));
    have = std::min<uint32_t>(cnt[0], (uint32_t) b->long_cap);
    overflow = cnt[1] || cnt[0] > (uint32_t) b->long_cap;
    return GNUAIS_OK;
}

extern "C" {

const char *gnuais_last_error(void) { return g_err.c_str(); }
const char *gnuais_version(void) { return "gnuais-hip 0.1 (gfx950)"; }

int gnuais_default_taps(float *out36)
{
    if (!out36) return fail(GNUAIS_E_ARG, "gnuais_default_taps: NULL");
    for (int k = 0; k < 18; ++k) {
        out36[k] = (float) k_tap_half[k];
        out36[35 - k] = (float) k_tap_half[k];
    }
    return 36;
}

// hand-off sets [sets_alloc, n): sign words, bit packs and their counts, K2b -> K3 slot ranges (zeroed)
static hipError_t alloc_sets(gnuais_batch *b, int n)
{
    const size_t N = (size_t) b->N;
    for (int k = b->sets_alloc; k < n && k < gnuais_batch::NBUF; ++k) {
        struct { Buf<uint32_t> &buf; size_t bytes; } want[] = {
            {b->sgn[k], sizeof(uint32_t) * sgn_words_alloc(b->sgn_words, b->N)},
            {b->segbits[k], sizeof(uint32_t) * N * (size_t) b->n_seg * PACK_STRIDE},
            {b->segcnt[k], sizeof(uint32_t) * N * (size_t) b->n_seg},
            {b->cand_first[k], sizeof(uint32_t) * N},
            {b->cand_count[k], sizeof(uint32_t) * N}};
        for (auto &w : want)                    // ensure: one may be left by an earlier attempt that failed further down this set
            if (hipError_t e = w.buf.ensure(w.bytes, true)) return e;
        b->sets_alloc = k + 1;
    }
    return hipSuccess;
}

void gnuais_batch_destroy(gnuais_batch *b)
{
    if (!b) return;
    (void) hipSetDevice(b->device);             // the owners release on the batch's device
    delete b;
}

int gnuais_batch_create(gnuais_batch **out, int device, int n_channels, const float *taps,
                        int n_taps, unsigned pllinc, int max_len, int frame_capacity)
{
    if (!out) return fail(GNUAIS_E_ARG, "create: out is NULL");
    *out = nullptr;
    if (n_channels <= 0 || max_len <= 0) return fail(GNUAIS_E_ARG, "create: n_channels/max_len");
    if (taps && (n_taps <= 0 || n_taps > GNUAIS_MAX_TAPS)) return fail(GNUAIS_E_ARG, "create: n_taps");
    if (pllinc > 0xffffu) return fail(GNUAIS_E_ARG, "create: pllinc must be < 0x10000");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(GNUAIS_E_HIP, "create: no HIP device");
    if (device < 0 || device >= ndev) return fail(GNUAIS_E_ARG, "create: device index");
    HIP_TRY(hipSetDevice(device));
    {   // the PLL stage keeps its position lists and bit packs in LDS (PLL_NEED_LDS, about 116 KB per workgroup) and
        // is compiled for gfx950's wave and LDS sizes only
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess &&
            lds < pll_need_lds())
            return fail(GNUAIS_E_HIP, "create: the device offers too little LDS per workgroup (gfx950 / MI355X with "
                                      "160 KB is what this library is built for)");
    }
    HIP_TRY(pll_prepare_device());              // per device: the PLL stage's LDS reservation

    gnuais_batch *b = new gnuais_batch;
    b->device = device;
    if (hipDeviceGetAttribute(&b->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || b->n_cu <= 0)
        b->n_cu = 256;
    b->N = n_channels;
    if (taps) {
        b->taps.assign(taps, taps + n_taps);
    } else {
        b->taps.resize(36);
        gnuais_default_taps(b->taps.data());
    }
    b->NT = (int) b->taps.size();
    b->pllinc = pllinc ? pllinc : (0x10000u / 5u);     // receiver.c:69
    b->max_len = max_len;
    b->frame_cap = frame_capacity > 0 ? frame_capacity : std::max(4096, n_channels * 48);

    // trim exactly-zero taps at both ends (exact, see fir_slice.hip)
    int k0 = 0, k1 = b->NT - 1;
    while (k0 < b->NT - 1 && b->taps[k0] == 0.0f) ++k0;
    while (k1 > k0 && b->taps[k1] == 0.0f) --k1;
    b->NE = k1 - k0 + 1;
    b->d = b->NT - k0;
    b->k0 = k0;
    if (b->NE <= FIR_MAX_NE)
        for (int j = 0; j < b->NE; ++j) b->te[j] = b->taps[k0 + j];

    b->sign = sign_bounds(b->te, b->NE);         // the sign-exact slicer's error bounds for this table (fir_plan.cpp)
    b->sgn_words = (max_len + 31) / 32;
    // at most one slice per sample step of (pllinc + pllinc/16)/65536
    const uint64_t step = (uint64_t) b->pllinc + b->pllinc / 16;
    b->bits_words = (int) (((uint64_t) max_len * step / 65536 + 2 + 31) / 32) + 1;

    const size_t N = (size_t) b->N;
    hipError_t e = hipSuccess;
    b->n_seg = (b->sgn_words + SEG_WORDS - 1) / SEG_WORDS;
    b->seg_words = (int) (((uint64_t) SEG_WORDS * 32 * step / 65536 + 2 + 31) / 32) + 1;
    // a frame start per 30 bits at most (see the candidate ring below), over the most bits ONE deframer launch can be
    // handed: what a run() call slices (bits_words), or the packs filled to their capacity by gnuais_batch_decode_bits()
    // (seg_words per segment: each pack is rounded up on its own, so n_seg of them hold more than the call's total)
    const uint64_t launch_bits = std::max((uint64_t) b->bits_words * 32, (uint64_t) b->seg_words * 32 * (uint64_t) b->n_seg);
    b->cand_K = (int) std::max<uint64_t>(64, launch_bits / 30 + 2);
    if (const char *v = getenv("GNUAIS_NBUF")) b->nbuf = std::min((int) gnuais_batch::NBUF, std::max(2, atoi(v)));
    {   // preflight: what this batch is about to allocate against what the device has free -- a batch that does not fit
        // says so with both figures at once instead of failing somewhere inside a dozen allocations
        const size_t per_set = sizeof(uint32_t) * (sgn_words_alloc(b->sgn_words, b->N) + N * (size_t) b->n_seg * (PACK_STRIDE + 1) + 2 * N);
        const size_t need = gnuais_batch::HB * (sizeof(int16_t) * N * b->NT + sizeof(int) * N) + (size_t) b->nbuf * per_set +
                            sizeof(uint32_t) * N * ((size_t) b->cand_K * CAND_WORDS + HDLC_CTL_WORDS + 6) +
                            sizeof(gnuais_frame) * (size_t) b->frame_cap;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
            char msg[256];
            snprintf(msg, sizeof msg, "create: %d channels x %d samples need %.2f GB of device memory, device %d has %.2f GB free of %.2f",
                     b->N, b->max_len, need / 1e9, device, free_b / 1e9, total_b / 1e9);
            delete b;
            return fail(GNUAIS_E_HIP, msg);
        }
    }
    auto alloc = [&](auto &buf, size_t bytes) {
        if (e == hipSuccess) e = buf.alloc(bytes, true);
    };
    for (int q = 0; q < gnuais_batch::HB; ++q) alloc(b->hist[q], sizeof(int16_t) * N * b->NT);
    if (b->seg_words > 16) {       // K2b keeps one segment pack (<= 16 words) in registers
        gnuais_batch_destroy(b);
        return fail(GNUAIS_E_ARG, "create: pllinc too large (more than one slice per ~4.6 samples)");
    }
    // the hand-off sets in use (`nbuf`; more are allocated when set_option raises it: a C5 set is 0.4 GB of sign words)
    if (e == hipSuccess) e = alloc_sets(b, b->nbuf);
    alloc(b->pll, sizeof(uint32_t) * N);
    alloc(b->lastbit, sizeof(uint32_t) * N);
    alloc(b->prev, sizeof(uint32_t) * N);
    alloc(b->ctl, sizeof(uint32_t) * N * HDLC_CTL_WORDS);
    // candidate ring, per channel and call.  The deframer cannot open frames faster than one per
    // 30 bits (16 alternating bits to leave ST_SKURR, protodec.c:1030-1043, six ones each for the
    // opening and the closing flag, a bit in ST_STOPSIGN), so this many slots hold whatever a call
    // can produce, adversarial bit streams included (real traffic: <= 38 frames per second)
    alloc(b->cand, sizeof(uint32_t) * N * (size_t) b->cand_K * CAND_WORDS);
    alloc(b->ring_count[0], sizeof(uint32_t) * 4);
    alloc(b->counters, sizeof(int32_t) * N * 3);
    for (int q = 0; q < gnuais_batch::HB; ++q) alloc(b->maxval[q], sizeof(int) * N);
    alloc(b->ring[0], sizeof(gnuais_frame) * (size_t) b->frame_cap);
    alloc(b->d_taps, sizeof(float) * b->NT);
    alloc(b->iq_prev, sizeof(int16_t) * 2 * N);
    if (b->sign.mfma_ok) {
        MfmaTaps host;
        fir_sign_mfma_pack(b->sign.tq, b->sign.tq_sum, &host);
        alloc(b->d_mfma, sizeof(MfmaTaps));
        if (e == hipSuccess) e = hipMemcpy(b->d_mfma, &host, sizeof(MfmaTaps), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = hipMemcpy(b->d_taps, b->taps.data(), sizeof(float) * b->NT, hipMemcpyHostToDevice);
    for (auto &set : b->evr)
        for (auto &ev : set)
            if (e == hipSuccess) e = ev.ensure();
    for (auto &pair : b->e_done)
        for (auto &ev : pair)
            if (e == hipSuccess) e = ev.ensure(hipEventDisableTiming);
    {
        // the sequential stages are short on parallelism, long on latency: give them
        // dispatch priority over the FIR's tens of thousands of workgroups
        int lo = 0, hi = 0;
        if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        // Creation order matters (measured, scripts/alloc_experiment.py + scripts/queue_ids.py):
        // HIP hands out hardware queues in creation order and the queues are spread over the
        // compute pipes round-robin, so in a process with no other streams the 4th stream
        // created here shares its pipe with the caller's (FIR) queue.  With the PLL stage or
        // the deframer there a C3 call takes 0.81-0.83 ms, with K3 there 0.90-0.93 (K3 is the
        // stage whose completion the host waits on before it reuses a hand-off set), with the spare
        // stream there 0.87.  That was with four streams per batch; with the twelve of the pool below the picture turns
        // (round 6, four fresh processes, C3: the PLL stage on the fourth stream 0.65-0.67 ms per step, on the first 0.503 =
        // what gnuais_batch_autotune() finds, 0.498-0.505; profiles/r06_stream_assignment.txt).  Hence: the PLL stage first,
        // then the spare, K2b, K3.  GNUAIS_STREAM_ORDER (four digits, stage indices 0 = K2 .. 3 = K3 in creation order)
        // overrides, for processes that have created streams of their own before.
        const char *order = getenv("GNUAIS_STREAM_ORDER");
        if (!order || strlen(order) != 4) order = "0123";
        int made = 0;
        for (int q = 0; q < 4; ++q) {
            const int idx = (order[q] - '0') & 3;
            if (e == hipSuccess && !b->s_k[idx]) {
                e = b->pool[made].ensure(hi);
                b->s_k[idx] = b->pool[made++];
            }
        }
        for (auto &st : b->s_k)
            if (e == hipSuccess && !st) {
                e = b->pool[made].ensure(hi);
                st = b->pool[made++];
            }
        for (int q = 0; q < 4; ++q) b->s_k_default[q] = b->s_k[q];
        // spare candidates for gnuais_batch_autotune(): in a process that has created streams of its
        // own the default assignment can be 1.7x slower than the best one (0.86 vs 1.39-1.43 ms
        // per C3 call with two application streams), and there is no API to ask which queue a
        // stream got -- so the assignment can be measured instead
        for (; made < gnuais_batch::POOL; ++made)
            if (e == hipSuccess) e = b->pool[made].ensure(made < 8 ? hi : 0);
    }
    if (const char *v = getenv("GNUAIS_K3_SAME")) b->k3_same = atoi(v) != 0;
    if (const char *v = getenv("GNUAIS_CYCLE")) b->cycle_parts = atoi(v) & 3;
    if (const char *v = getenv("GNUAIS_PLL_VARIANT")) {      // the values set_option takes, nothing else
        const int pv = atoi(v);
        if (pv == 0 || pv == 7 || pv == 8) b->pll_variant = pv;
    }
    if (const char *v = getenv("GNUAIS_PIPELINE")) b->pipeline = atoi(v) != 0;
    if (const char *v = getenv("GNUAIS_HDLC_VARIANT")) b->hdlc_variant = atoi(v) != 0;
    if (const char *v = getenv("GNUAIS_HDLC_LPW")) b->hdlc_lpw = std::min(64, std::max(1, atoi(v)));
    if (e != hipSuccess) {
        gnuais_batch_destroy(b);
        return fail(GNUAIS_E_HIP, "create: device allocation", e);
    }
    if (const char *v = getenv("GNUAIS_FIR_VARIANT")) {
        const int fv = atoi(v);
        if (fv == 0 || fv == 3) b->fir.fir_variant = fv;
    }
    if (const char *v = getenv("GNUAIS_FIR_FLAG2")) b->fir.fir_flag2 = atoi(v) != 0;
    if (const char *v = getenv("GNUAIS_FIR_T")) b->fir.fir_T = std::max(64, atoi(v) / 32 * 32);
    *out = b;
    int rc = gnuais_batch_reset(b);
    if (rc != GNUAIS_OK) {
        gnuais_batch_destroy(b);
        *out = nullptr;
    }
    return rc;
}


// the frame rings back to their start: every ring that exists empty and idle, K3 on ring 0 (the device is idle)
static int rings_reset(gnuais_batch *b)
{
    for (int q = 0; q < gnuais_batch::NRING; ++q) {
        if (b->ring_count[q]) HIP_TRY(hipMemset(b->ring_count[q], 0, sizeof(uint32_t) * 4));
        b->s_stage[q] = 0;
        b->ring_runs[q] = 0;
    }
    b->ring_cur = 0;
    b->stream_calls = 0;
    b->discard_pending = false;                 // every word of every ring is zero
    return GNUAIS_OK;
}

// D' of gnuais_batch_long_frames back to protodec_reset()'s state, a frame in progress dropped (the device is idle or the
// null stream orders it); everything: also its two counters and its ring
static int long_zero_state(gnuais_batch *b, bool everything)
{
    if (!b->long_ctl) return GNUAIS_OK;         // never switched on: nothing exists
    HIP_TRY(launch_hdlc_long_reset(b->long_ctl, everything ? b->long_counters.p : nullptr, b->N, nullptr));
    if (everything) HIP_TRY(hipMemset(b->long_count, 0, sizeof(uint32_t) * 2));
    // the candidate ring of gnuais_batch_long_repair is empty between calls (consumed within each); a frame in progress
    // restarts with its record, so nothing of it needs clearing.  Both counters and the parity start over all the same.
    if (everything && b->long_cand_count) {
        HIP_TRY(hipMemset(b->long_cand_count, 0, sizeof(uint32_t) * 2));
        b->long_parity = 0;
    }
    return GNUAIS_OK;
}

// what is latched from the row count when it is set -- to 0 by a reset, to any row by gnuais_batch_set_clock
static int latch_rows(gnuais_batch *b, unsigned long long rows)
{
    b->rows = rows;
    b->fs_v0 = b->fs_end = rows;                // gnuais_batch_frame_signal: a new run of I/Q-type calls starts at this row
    return occ_zero_state(b);                   // gnuais_batch_occupancy: and its epochs count from there, the queue is empty
}

int gnuais_batch_reset(gnuais_batch *b)
{
    if (!b) return fail(GNUAIS_E_ARG, "reset: NULL batch");
    if (int rc = set_device(b)) return rc;
    const size_t N = (size_t) b->N;
    if (int rc = discard_flush(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int q = 0; q < gnuais_batch::HB; ++q)
        HIP_TRY(hipMemset(b->hist[q], 0, sizeof(int16_t) * N * b->NT));   // filter.c:62
    b->hist_cur = 0;
    HIP_TRY(hipMemset(b->pll, 0, sizeof(uint32_t) * N));              // receiver.c:66-71
    HIP_TRY(hipMemset(b->lastbit, 0, sizeof(uint32_t) * N));
    HIP_TRY(hipMemset(b->prev, 0, sizeof(uint32_t) * N));
    for (int k = 0; k < b->sets_alloc; ++k)
        HIP_TRY(hipMemset(b->segcnt[k], 0, sizeof(uint32_t) * N * (size_t) b->n_seg));
    b->calls = 0;
    if (int rc = latch_rows(b, 0)) return rc;
    b->last[CHAIN].used = false;
    b->hdlc_calls = 0;
    HIP_TRY(hipMemset(b->counters, 0, sizeof(int32_t) * N * 3));      // protodec.c:62-64
    if (b->repaired) HIP_TRY(hipMemset(b->repaired, 0, sizeof(int32_t) * N));
    b->uq.n_tail = 0;                           // gnuais_batch_unique: no open cluster, nothing late (the window stays)
    b->uq.late = 0;
    b->lq.n_tail = 0;                           // gnuais_batch_long_unique: likewise, a state of its own
    b->lq.late = 0;
    for (int q = 0; q < gnuais_batch::HB; ++q) HIP_TRY(hipMemset(b->maxval[q], 0, sizeof(int) * N));
    b->max_cur = 0;
    b->max_last = 0;
    if (int rc = rings_reset(b)) return rc;
    for (auto &p : b->sd_seq)
        if (p) HIP_TRY(hipMemset(p, 0, N));
    HIP_TRY(launch_hdlc_reset(b->ctl, b->N, nullptr));                // protodec.c:87-100
    if (int rc = long_zero_state(b, true)) return rc;                 // gnuais_batch_long_frames: D', its counters, its ring
    HIP_TRY(hipMemset(b->iq_prev, 0, sizeof(int16_t) * 2 * N));       // the discriminator's previous pair: (0, 0)
    b->last[DISC].used = false;
    if (int rc = chan_zero_state(b)) return rc;
    if (int rc = afc_zero_state(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->last_len = 0;
    b->pll_form = 0;
    b->clock_fresh = true;
    return GNUAIS_OK;
}

// The clocks of a batch that has taken nothing since create / reset, set as if that reset had happened at row `rows`
// with h_bits[c] bits fed on channel c: the row count and what reset latches from it, and the deframer's bit count
int gnuais_batch_set_clock(gnuais_batch *b, long long rows, const uint64_t *h_bits)
{
    if (!b) return fail(GNUAIS_E_ARG, "set_clock: NULL batch");
    if (rows < 0) return fail(GNUAIS_E_ARG, "set_clock: rows < 0");
    if (!b->clock_fresh) return fail(GNUAIS_E_STATE, "set_clock: a run or decode call has been made since create / reset");
    if (b->wide.K || b->afc_W)
        return fail(GNUAIS_E_STATE, "set_clock: not with a wide stage or the AFC configured (their sample counts start at 0)");
    if (int rc = set_device(b)) return rc;
    const size_t N = (size_t) b->N;
    std::vector<uint32_t> lo(N), hi(N);
    for (size_t c = 0; c < N; ++c) {
        const uint64_t v = h_bits ? h_bits[c] : 0;
        lo[c] = (uint32_t) v;
        hi[c] = (uint32_t) (v >> 32);           // every bit, as the deframer stores it
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(b->ctl + 2 * N, lo.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->ctl + 5 * N, hi.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice));
    return latch_rows(b, (unsigned long long) rows);        // the same code reset uses
}

int gnuais_batch_set_option(gnuais_batch *b, const char *name, int value)
{
    if (!b || !name) return fail(GNUAIS_E_ARG, "set_option: NULL");
    if (!strcmp(name, "stage_mask")) {          // timing experiments; results are invalid if != 0x1f
        b->stage_mask = value & 0x1f;
        return GNUAIS_OK;
    }
    if (!strcmp(name, "fir_T")) {
        if (value < 64 || value % 32) return fail(GNUAIS_E_ARG, "fir_T must be a multiple of 32, >= 64");
        b->fir.fir_T = value;
    } else if (!strcmp(name, "nbuf")) {             // hand-off sets in use: the calls that may be in flight
        if (value < 2 || value > gnuais_batch::NBUF) return fail(GNUAIS_E_ARG, "nbuf must be 2..8");
        if (b->frame_signal && value > b->fs_nbuf)
            return fail(GNUAIS_E_STATE, "nbuf: the block ring of gnuais_batch_frame_signal is sized for the depth it was switched on "
                                        "at; switch it off first");
        if (b->occ_E && value > b->occ_nbuf)
            return fail(GNUAIS_E_STATE, "nbuf: the rings of gnuais_batch_occupancy are sized for the depth it was switched on at; "
                                        "switch it off first");
        if (int rc = gnuais_batch_sync(b)) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(alloc_sets(b, value));
        b->nbuf = value;
    } else if (!strcmp(name, "streaming")) {
        // 0: leave the streamed delivery (gnuais_batch_stream_nmea / autotune_delivery switch it on): everything in
        // flight is flushed and DROPPED, K3 goes back to ring 0, the drain-type calls work again.  The rings, texts
        // and streams stay allocated for the next streaming call.
        if (value != 0 && b->frame_times)
            return fail(GNUAIS_E_STATE, "streaming: the batch times its frames (gnuais_batch_frame_times); the streamed delivery carries no times");
        if (value != 0 && b->repair)
            return fail(GNUAIS_E_STATE, "streaming: the batch repairs frames (gnuais_batch_repair); the streamed delivery's order table describes the CRC stage's records only");
        if (value != 0 && b->frame_signal)
            return fail(GNUAIS_E_STATE, "streaming: the batch measures its frames (gnuais_batch_frame_signal); the streamed delivery carries no records of them");
        if (value != 0 && b->uq.window)
            return fail(GNUAIS_E_STATE, "streaming: the batch merges duplicates (gnuais_batch_unique); the streamed delivery has no such stage");
        if (value != 0 && b->long_repair)
            return fail(GNUAIS_E_STATE, "streaming: the batch repairs long frames (gnuais_batch_long_repair); the streamed delivery carries no records of them");
        if (value != 0 && b->long_frames)
            return fail(GNUAIS_E_STATE, "streaming: the batch decodes long frames (gnuais_batch_long_frames); the streamed delivery carries no records of them");
        if (value != 0) return fail(GNUAIS_E_ARG, "streaming can only be switched off here (stream_nmea switches it on)");
        if (b->streaming) {
            if (int rc = gnuais_batch_sync(b)) return rc;
            HIP_TRY(hipDeviceSynchronize());
            if (int rc = rings_reset(b)) return rc;
            b->hdlc_calls = 0;
            b->streaming = false;
        }
    } else if (!strcmp(name, "fir_flag2")) {         // 0: |y| - eps and two alignbits per output (rounds 1-4)
        if (value != 0 && value != 1) return fail(GNUAIS_E_ARG, "fir_flag2: 0 or 1");
        b->fir.fir_flag2 = value;
    } else if (!strcmp(name, "fir_pk_taps")) {       // long tables: 0 = 40 central taps where the table allows them, 48 = never 40
        if (value != 0 && value != 48) return fail(GNUAIS_E_ARG, "fir_pk_taps: 0 or 48");
        b->fir.fir_pk_taps = value;
    } else if (!strcmp(name, "fir_mfma")) {          // long tables: 1 = inner segments on the matrix pipe (fir_sign_mfma.hip), 0 = the packed kernel throughout
        if (value != 0 && value != 1) return fail(GNUAIS_E_ARG, "fir_mfma: 0 or 1");
        b->fir.fir_mfma = value;
    } else if (!strcmp(name, "fir_variant")) {
        if (value != 0 && value != 3) return fail(GNUAIS_E_ARG, "fir_variant must be 0 (the exact sum for every sample) or 3 (the sign-exact slicer)");
        b->fir.fir_variant = value;
    } else if (!strcmp(name, "timing_stride")) {
        if (value < 1) return fail(GNUAIS_E_ARG, "timing_stride must be >= 1");
        b->timing_stride = value;
    } else if (!strcmp(name, "pipeline")) {
        if (int rc = discard_flush(b)) return rc;       // "behind the last K3" names another stream from here on
        b->pipeline = value != 0;
    } else if (!strcmp(name, "pll_variant")) {
        if (value != 0 && value != 7 && value != 8)
            return fail(GNUAIS_E_ARG, "pll_variant must be 0 (by channel count), 7 (time-parallel, pll_tp.hip) or 8 (pll_h3.hip)");
        b->pll_variant = value;
    } else if (!strcmp(name, "hdlc_variant")) {
        b->hdlc_variant = value != 0;
    } else if (!strcmp(name, "unique_hash_bits")) {  // tests: a truncated hash forces the duplicate merge's exact path
        if (value < 1 || value > 64) return fail(GNUAIS_E_ARG, "unique_hash_bits must be 1..64");
        b->uq_hash_bits = value;
    } else if (!strcmp(name, "hdlc_lpw")) {
        if (value < 1 || value > 64) return fail(GNUAIS_E_ARG, "hdlc_lpw must be 1..64");
        b->hdlc_lpw = value;
    } else {
        return fail(GNUAIS_E_ARG, "set_option: unknown option");
    }
    return GNUAIS_OK;
}

// everything of a FIR launch that is not a decision: buffers, taps, shape
static void fill_fir(const gnuais_batch *b, FirLaunch &f, const int16_t *x, int len, float *dump,
                     int k)
{
    memset(&f, 0, sizeof f);
    f.x = x;
    f.hist = b->hist[b->hist_cur];
    f.sgn = b->sgn[k];
    f.dump = dump;
    f.maxval = b->maxval[b->max_cur];
    f.hist_out = b->hist[(b->hist_cur + 1) % gnuais_batch::HB];
    f.maxval_next = b->maxval[(b->max_cur + 2) % gnuais_batch::HB];
    f.d_taps = b->d_taps;
    memcpy(f.te, b->te, sizeof f.te);
    f.N = b->N;
    f.L = len;
    f.NT = b->NT;
    f.NE = b->NE;
    f.d = b->d;
    f.te_mem = b->d_taps + b->k0;
    f.map = 1;                      // K1s workgroup mapping (fir_slice.hip): XCD-contiguous channel groups
}

static void fill_hdlc(const gnuais_batch *b, HdlcLaunch &h, int k)
{
    h.segbits = b->segbits[k]; h.segcnt = b->segcnt[k]; h.ctl = b->ctl; h.cand = b->cand;
    h.cand_first = b->cand_first[k]; h.cand_count = b->cand_count[k];
    h.counters = b->counters;
    h.frames = b->ring[b->ring_cur];
    h.frame_count = b->ring_count[b->ring_cur];
    h.frame_cap = (uint32_t) b->frame_cap; h.N = b->N; h.n_seg = b->n_seg;
    h.seg_words = b->seg_words; h.K = b->cand_K; h.K_call = b->cand_K;
    // event-driven deframer: 16 channels per wave finish a small batch soonest; where the chip is full anyway (a PLL
    // workgroup on every CU, four FIR waves per SIMD) 64 per wave -- a quarter of the waves -- cost the other stages
    // least: C3 steady state 0.492 against 0.525 ms per call (profiles/r05_pll_h3_in_the_pipeline.txt)
    // small batches: a lane's walk through its events is the stage's latency, and the fewer lanes share a wave the less
    // they wait for each other -- as few per wave as keep the launch at <= 512 waves (256 channels: 0.148 ms with one
    // lane per wave against 0.243 with 16; 1024 channels: 0.180 with two, 0.216 with one; time_pll_forms.py, round 5)
    int small_lpw = 1;
    while (small_lpw < 16 && (b->N + small_lpw - 1) / small_lpw > 512) small_lpw *= 2;
    if (b->N > PLL_TP_MAX_CHANNELS) small_lpw = 16;      // beside the lane-per-channel PLL more deframer waves cost more than they save (2048 channels: 0.346 against 0.336 ms per call)
    const int ev_lpw = 2 * ((b->N + 63) / 64) > (b->n_cu > 0 ? b->n_cu : 256) ? 64 : small_lpw;
    h.lanes_per_wave = b->hdlc_lpw ? b->hdlc_lpw : (b->hdlc_variant ? ev_lpw : 64);
    // the chunk table describes ONE launch; a second one into the same ring would overwrite it
    h.chunks = (b->streaming && b->ring_runs[b->ring_cur] == 0) ? b->ring_chunks[b->ring_cur] : nullptr;
    // a pending gnuais_batch_discard_frames rides on this launch's deframer (a batch that streams takes no discard)
    h.discard = b->discard_pending && !b->streaming && b->ring_cur == 0;
    h.ovf_mark = 2u << ((b->discard_launches + (h.discard ? 1u : 0u)) & 1u);
}

// the deframer launch described by h; a discard it carried is no longer pending
static int run_deframer(gnuais_batch *b, const HdlcLaunch &h, hipStream_t s)
{
    HIP_TRY(b->hdlc_variant ? launch_hdlc_events(h, s) : launch_hdlc_deframe(h, s));
    if (h.discard) {
        b->discard_pending = false;
        b->discard_launches++;
    }
    return GNUAIS_OK;
}

// the launch behind the K3 described by h: len rows from row b->rows on (len <= 0: bits without samples)
static FrameTimeLaunch fill_frame_times(const gnuais_batch *b, const HdlcLaunch &h, int len)
{
    FrameTimeLaunch t;
    t.frames = h.frames; t.frame_count = h.frame_count; t.frame_cap = h.frame_cap;
    t.ctl = h.ctl; t.segcnt = h.segcnt; t.times = b->times;
    t.N = h.N; t.n_seg = h.n_seg; t.seg_words = h.seg_words;
    t.len = len; t.n0 = (int64_t) b->rows;
    return t;
}

// the launch behind that one: the records of a call that did not come through run_form (fs_iq_call) get (0, 0, 0) --
// v0 behind its last row
static FrameSignalLaunch fill_frame_signal(const gnuais_batch *b, const HdlcLaunch &h, int len)
{
    FrameSignalLaunch a;
    a.frames = h.frames; a.frame_count = h.frame_count; a.frame_cap = h.frame_cap;
    a.times = b->times; a.ring = b->fs_ring; a.signal = b->signal.p;
    a.RB = b->fs_RB; a.N = h.N;
    a.len = len; a.n0 = (int64_t) b->rows;
    a.pllinc = b->pllinc; a.n_taps = b->NT; a.afc_window = b->afc_W;
    a.v0 = (int64_t) (b->fs_iq_call ? b->fs_v0 : b->rows + (unsigned long long) std::max(len, 0));
    return a;
}

// the launch behind the K3 described by h, in front of its frame_time launch
static RepairLaunch fill_repair(const gnuais_batch *b, const HdlcLaunch &h)
{
    RepairLaunch r;
    r.cand = h.cand; r.cand_first = h.cand_first; r.cand_count = h.cand_count;
    r.repaired = b->repaired;
    r.frames = h.frames; r.frame_count = h.frame_count; r.frame_cap = h.frame_cap;
    r.N = h.N; r.K = h.K;
    return r;
}

// the launch behind the K3 described by h: D' over the same packs, len rows from row b->rows on (len <= 0: bits without
// samples)
static LongLaunch fill_long(const gnuais_batch *b, const HdlcLaunch &h, int len)
{
    LongLaunch a;
    a.segbits = h.segbits; a.segcnt = h.segcnt; a.ctl = h.ctl;
    a.lctl = b->long_ctl; a.open = b->long_open; a.counters = b->long_counters;
    a.frames = b->long_ring.p; a.frame_count = b->long_count; a.frame_cap = (uint32_t) b->long_cap;
    a.N = h.N; a.n_seg = h.n_seg; a.seg_words = h.seg_words;
    a.len = len; a.n0 = (int64_t) b->rows;
    if (b->long_repair) {                       // the form that keeps the raw bits and lists the failed frames
        a.clean = b->long_clean; a.cand = b->long_cand; a.cand_count = b->long_cand_count;
        a.cand_cap = (uint32_t) b->long_cand_cap; a.parity = b->long_parity;
    }
    return a;
}

// D' behind the K3 described by h and, while gnuais_batch_long_repair is on, the repair of what it counted in `failed`
// behind it on the same stream; the next call counts its candidates in the other word
static int run_long(gnuais_batch *b, const HdlcLaunch &h, int len, hipStream_t s)
{
    HIP_TRY(launch_hdlc_long(fill_long(b, h, len), s));
    if (b->long_repair) {
        LongRepairLaunch r;
        r.cand = b->long_cand; r.cand_count = b->long_cand_count.p + b->long_parity; r.cand_cap = (uint32_t) b->long_cand_cap;
        r.repaired = b->long_counters.p + 2 * (size_t) b->N;
        r.frames = b->long_ring.p; r.frame_count = b->long_count; r.frame_cap = (uint32_t) b->long_cap;
        r.N = b->N;
        r.blocks = 16 * std::max(b->n_cu, 1);   // four waves per SIMD: fixed, the count is known on the device only
        HIP_TRY(launch_hdlc_long_repair(r, s));
        b->long_parity ^= 1;
    }
    return GNUAIS_OK;
}

// K1 + carry: the kernel and its thresholds are plan_fir()'s choice (fir_plan.cpp).  The specialised kernels update
// the history and clear the next peak buffer themselves; the generic fallback needs the two helper launches.
static int run_fir(gnuais_batch *b, const int16_t *x, int len, float *dump, hipStream_t s, int k)
{
    const FirPlan p = plan_fir(b->sign, b->fir, FirShape{b->N, b->NT, b->NE, b->d}, len, dump != nullptr);
    FirLaunch f;
    fill_fir(b, f, x, len, dump, k);
    static_cast<FirThresholds &>(f) = p.th;
    if (b->sign.ok)
        for (int j = 0; j < f.NC; ++j) f.ctaps[j] = b->te[(b->NE - f.NC) / 2 + j];
    switch (p.kernel) {
    case FirKernel::GENERIC:
        HIP_TRY(hipMemsetAsync(f.maxval_next, 0, sizeof(int) * (size_t) b->N, s));
        HIP_TRY(launch_fir_generic(f, s));
        HIP_TRY(launch_fir_history(x, f.hist, f.hist_out, b->N, len, b->NT, s));
        break;
    case FirKernel::SCALAR32:
        HIP_TRY(scalar::launch_fir_slice(f, s));
        break;
    case FirKernel::SIGN:
        HIP_TRY(launch_fir_sign(f, s));
        break;
    case FirKernel::SIGN_PACKED:
        HIP_TRY(launch_fir_sign_pk(f, s));
        break;
    case FirKernel::SIGN_PACKED_MFMA: {
        FirLaunch m = f;            // the matrix pipe behind the packed kernel's head, its thresholds in ITS units
        f.T = p.head;
        f.max_segments = 1;
        m.NC = FIR_MFMA_NC;
        m.mfma = b->d_mfma;
        m.eps_seen = p.mfma_seen_u;
        m.eps_ahead = p.mfma_abs_u;
        HIP_TRY(launch_fir_sign_pk(f, s));
        HIP_TRY(launch_fir_sign_mfma(m, p.head, s));
        break;
    }
    }
    b->hist_cur = (b->hist_cur + 1) % gnuais_batch::HB;
    b->max_last = b->max_cur;
    b->max_cur = (b->max_cur + 1) % gnuais_batch::HB;
    return GNUAIS_OK;
}

static void fill_pll(const gnuais_batch *b, PllLaunch &p, int k, int len)
{
    p.sgn = b->sgn[k]; p.pll = b->pll; p.prev = b->prev;
    p.watchdog = b->ring_count[b->ring_cur] + 3; p.lastbit = b->lastbit;
    p.segbits = b->segbits[k]; p.segcnt = b->segcnt[k];
    p.N = b->N; p.L = len; p.n_seg = b->n_seg; p.seg_words = b->seg_words; p.pllinc = b->pllinc; p.variant = b->pll_variant;
    p.n_cu = b->n_cu;
}


// K2b, K3 of one call, each on its own stream (pipeline) or all on s0, after `after`
// (the event that says this call's PLL stage is done; null = stream order on s0).
static int run_tail(gnuais_batch *b, int k, int len, bool tm, const Event *ev,
                    hipStream_t s0, hipEvent_t after)
{
    const bool pl = b->pipeline;
    hipStream_t sC = pl ? b->s_k[2] : s0, sD = pl ? k3_stream(b) : s0;
    HdlcLaunch h;
    fill_hdlc(b, h, k);
    // K2b: needs segbits[k]; fills cand_first/count[k] (read by K3 of call - NBUF).  It also writes
    // the per-channel candidate ring that K3 of the PREVIOUS call may still be reading: slots are
    // reused after cand_K frame starts, which one call cannot exceed but two could
    if (pl && after) HIP_TRY(hipStreamWaitEvent(sC, after, 0));
    if (pl && b->calls >= 1 && sD != sC)
        HIP_TRY(hipStreamWaitEvent(sC, b->e_done[4][(k + b->nbuf - 1) % b->nbuf], 0));
    if (tm) HIP_TRY(hipEventRecord(ev[5], sC));
    if (b->stage_mask & 8)
        if (int rc = run_deframer(b, h, sC)) return rc;
    if (tm) HIP_TRY(hipEventRecord(ev[7], sC));
    // e_done[3][k] has one waiter: the K3 of this call, when it runs on a stream of its own.  On the deframer's stream
    // the order is the stream's, and the record would be one more packet between the two launches of the serial cycle.
    const bool hand_off = pl && (sD != sC || !(b->cycle_parts & 2));
    if (hand_off) HIP_TRY(hipEventRecord(b->e_done[3][k], sC));
    // K3
    if (pl && sD != sC) HIP_TRY(hipStreamWaitEvent(sD, b->e_done[3][k], 0));
    // a discard still pending here found no deframer launch to ride on (stage_mask): the memset, where it always was
    if (int rc = discard_flush(b)) return rc;
    if (tm) HIP_TRY(hipEventRecord(ev[9], sD));
    if (b->stage_mask & 16) HIP_TRY(launch_hdlc_crc(h, sD));
    // the repair of what K3 counted in lostframes: behind K3, in front of the times (repaired frames get theirs) and of
    // e_done[4][k], which is what the reuse of set k (cand_first, cand_count) and, where K3 has a stream of its own, the
    // next deframer launch (the candidate slots) wait for
    if (b->repair && (b->stage_mask & 16)) HIP_TRY(launch_hdlc_repair(fill_repair(b, h), sD));
    // the frames' receive times: behind K3 and in front of e_done[4][k], which is what the reuse of set k (segcnt) and,
    // where K3 has a stream of its own, the next deframer launch (ctl) wait for
    if (b->frame_times && (b->stage_mask & 16)) HIP_TRY(launch_frame_times(fill_frame_times(b, h, len), sD));
    // their power and carrier error: behind the times it selects its records by, in front of e_done[4][k] (frame_signal.hip)
    if (b->frame_signal && (b->stage_mask & 16)) HIP_TRY(launch_frame_signal(fill_frame_signal(b, h, len), sD));
    // the channels' load: the cover of this call's frames behind their times, then the epochs the call makes final, in
    // front of e_done[4][k] (occupancy.hip; only a call that came through run_form has I/Q rows)
    // Where the long frames cover too (gnuais_batch_long_frame_signal), the finalisers wait for their cover launch: chain
    // cover, D', long repair, long signal and cover, then the finalisers.  Else the sequence is the one it always was.
    const bool occ = b->occ_E && b->fs_iq_call && (b->stage_mask & 16);
    const bool long_sig = b->long_frames && b->long_frame_signal && (b->stage_mask & 8);
    if (occ) {
        if (int rc = occ_cover(b, h, len, sD)) return rc;
        if (!long_sig)
            if (int rc = occ_finalise(b, len, sD)) return rc;
    }
    // messages of three to five slots: D' over this call's packs, behind the deframer that moved the bit count it reads
    // and in front of e_done[4][k], which is what the reuse of set k (segbits, segcnt) and, where K3 has a stream of its
    // own, the next deframer launch (ctl) wait for (hdlc_long.hip)
    if (b->long_frames && (b->stage_mask & 8))
        if (int rc = run_long(b, h, len, sD)) return rc;
    // their power and carrier error, and their cover: behind D' and the long repair, which append the records, and in
    // front of e_done[4][k] (long_signal.hip)
    if (long_sig) {
        HIP_TRY(launch_long_signal(long_signal_launch(b, len), sD));
        if (occ)
            if (int rc = occ_finalise(b, len, sD)) return rc;
    }
    if (b->streaming) b->ring_runs[b->ring_cur]++;
    b->hdlc_calls++;
    if (tm) HIP_TRY(hipEventRecord(ev[4], sD));
    if (pl) HIP_TRY(hipEventRecord(b->e_done[4][k], sD));
    return GNUAIS_OK;
}

int gnuais_batch_run(gnuais_batch *b, const int16_t *d_samples, int len, void *stream)
{
    if (!b || !d_samples) return fail(GNUAIS_E_ARG, "run: NULL argument");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "run: len out of range (max_len)");
    if (int rc = set_device(b)) return rc;
    b->clock_fresh = false;
    hipStream_t s0 = (hipStream_t) stream;
    const bool pl = b->pipeline;
    const int k = (int) (b->calls % (unsigned) b->nbuf);      // hand-off buffer set of this call
    const bool reuse = pl && b->calls >= (unsigned) b->nbuf;  // set k last used by call i-nbuf
    const bool tm = b->timing && (b->calls % (unsigned) b->timing_stride) == 0;
    const Event *ev = b->evr[b->timed_calls % gnuais_batch::TIMING_RING];

    {
        hipStream_t sA = pl ? b->s_k[0] : s0;
        // Hand-off set k was last used by call i-nbuf.  Its last user is that call's K3; wait for
        // it on the HOST (normally long done): five stream-wait packets per call, each ~20 us of
        // queue time on the stream it sits in, for a condition that is practically always true.
        // A caller that runs more than nbuf-1 calls ahead of the device blocks here.  (Round 4, measured once more at
        // depth 3, where this wait IS the loop: ONE wait packet on the caller's stream instead, the host held back only
        // by that call's FIR launch -- 0.583 against 0.542 ms per step, profiles/r04_k3_on_the_deframers_stream.txt.)
        if (reuse) HIP_TRY(hipEventSynchronize(b->e_done[4][k]));
        // K1 carries the FIR history and the peak buffers from call to call in stream order (the drain rule)
        if (int rc = drain(b, 1u << CHAIN, s0)) return rc;
        hipStream_t sF = s0;
        if (tm) HIP_TRY(hipEventRecord(ev[0], sF));
        if (b->stage_mask & 1)
            if (int rc = run_fir(b, d_samples, len, nullptr, sF, k)) return rc;
        if (tm) HIP_TRY(hipEventRecord(ev[1], sF));
        if (b->e_in_hook) {                     // run_host_async: its staging pair is free once K1 has read it --
            HIP_TRY(hipEventRecord(b->e_in_hook, sF));      // also when the whole chain runs on this one stream
            b->e_in_hook = nullptr;
        }
        if (pl) HIP_TRY(hipEventRecord(b->e_done[0][k], sF));
        // K2: this call's sign words -> bit packs segbits[k] (read by K2b of call i-nbuf); in order
        // across calls (it carries the receivers' pll / prev / lastbit)
        PllLaunch p;
        fill_pll(b, p, k, len);
        if (pl) HIP_TRY(hipStreamWaitEvent(sA, b->e_done[0][k], 0));
        if (tm) HIP_TRY(hipEventRecord(ev[2], sA));
        if (b->stage_mask & 2) {
            b->pll_form = pll_form_of(p);       // info "pll_form": the form launch_pll() takes for these arguments
            HIP_TRY(launch_pll(p, sA));
        }
        if (tm) HIP_TRY(hipEventRecord(ev[6], sA));
        if (pl) HIP_TRY(hipEventRecord(b->e_done[1][k], sA));
        if (int rc = run_tail(b, k, len, tm, ev, s0, pl ? b->e_done[1][k] : nullptr)) return rc;
    }

    b->timed_last = tm;
    if (tm) b->timed_calls++;
    b->last[CHAIN] = {s0, true};
    b->last_len = len;
    b->last_k = k;
    b->calls++;
    b->rows += (unsigned long long) len;
    return GNUAIS_OK;
}

// Try the stage -> stream assignments greedily (PLL stage first, then K3, K2b, the spare; each on every
// free candidate stream), timing a few pipelined calls of the caller's own input each, and keep
// the fastest.  Resets the batch afterwards (the calls advanced every receiver's state).
int gnuais_batch_autotune(gnuais_batch *b, const int16_t *d_samples, int len, void *stream, float *ms_per_call)
{
    if (!b || !d_samples) return fail(GNUAIS_E_ARG, "autotune: NULL argument");
    if (!b->pipeline) {                         // one stream, nothing to assign
        if (ms_per_call) *ms_per_call = 0.0f;
        return GNUAIS_OK;
    }
    if (int rc = gnuais_batch_sync(b)) return rc;
    const bool timing = b->timing;
    b->timing = false;
    // the assignment is measured with K3 on a stream of its own (role 3 gets a queue that was timed: the streamed
    // delivery runs K3 there); outside the delivery loop K3 then shares the deframer's stream (k3_same)
    struct K3Own { gnuais_batch *b; int was; ~K3Own() { b->k3_same = was; } } k3_own{b, b->k3_same};
    b->k3_same = 0;
    auto measure = [&](double &ms, int meas = 10) -> int {
        const int warm = 4;
        for (int i = 0; i < warm + meas; ++i) {
            if (i == warm) {
                if (int rc = gnuais_batch_sync(b)) return rc;
                ms = -now_ms();
            }
            if (int rc = gnuais_batch_run(b, d_samples, len, stream)) return rc;
            if (int rc = gnuais_batch_discard_frames(b, stream)) return rc;
        }
        if (int rc = gnuais_batch_sync(b)) return rc;
        ms = (ms + now_ms()) / meas;
        return GNUAIS_OK;
    };
    const int order[4] = {0, 3, 2, 1};          // the PLL stage first, then K3, K2b, the spare
    double best_all = 0;
    auto search = [&](int chosen[4]) -> int {
        for (int q = 0; q < 4; ++q) chosen[q] = -1;
        for (int r = 0; r < 4; ++r) {
            const int role = order[r];
            double best = 1e30;
            int best_s = -1;
            for (int cand = 0; cand < gnuais_batch::POOL; ++cand) {
                bool used = false;
                for (int q = 0; q < r; ++q) used |= chosen[order[q]] == cand;
                if (used) continue;
                int trial[4];
                for (int q = 0; q < 4; ++q) trial[q] = chosen[q];
                trial[role] = cand;
                for (int q = r + 1; q < 4; ++q) {   // the roles not decided yet: any distinct free streams
                    for (int f = 0; f < gnuais_batch::POOL; ++f) {
                        bool taken = false;
                        for (int t = 0; t < 4; ++t) taken |= trial[t] == f;
                        if (!taken) { trial[order[q]] = f; break; }
                    }
                }
                for (int q = 0; q < 4; ++q) b->s_k[q] = b->pool[trial[q]];
                double ms = 0;
                if (int rc = measure(ms)) return rc;
                if (ms < best) { best = ms; best_s = cand; }
            }
            chosen[role] = best_s;
        }
        return GNUAIS_OK;
    };
    // Ten calls per trial are noisy (+-4 %) and a greedy search can follow the noise into a poor
    // assignment (seen: 0.65 instead of 0.53 ms per call in a third of the runs on one box).  So: two
    // independent searches, and the default assignment, in a longer head-to-head; the fastest stays.
    hipStream_t cand_set[3][4];
    int n_sets = 0;
    for (int q = 0; q < 4; ++q) cand_set[0][q] = b->s_k_default[q];
    n_sets = 1;
    for (int rep = 0; rep < 2; ++rep) {
        int chosen[4];
        if (int rc = search(chosen)) return rc;
        for (int q = 0; q < 4; ++q) cand_set[n_sets][q] = b->pool[chosen[q]];
        ++n_sets;
    }
    // The default assignment (creation order, see gnuais_batch_create) is the best one wherever the process has created no
    // streams of its own (round 6, three boxes: un-calibrated within 1 % of the best calibrated run) and a 40-call leg
    // still carries +-2 % of noise, so a searched assignment only replaces it when it is at least 3 % faster: what a
    // plain gnuais_batch_run() caller gets is then never worse than what this call leaves behind.
    int best_set = 0;
    best_all = 1e30;
    double ms_set[3] = {0, 0, 0};
    for (int k = 0; k < n_sets; ++k) {
        for (int q = 0; q < 4; ++q) b->s_k[q] = cand_set[k][q];
        if (int rc = measure(ms_set[k], 40)) return rc;
    }
    best_all = ms_set[0];
    for (int k = 1; k < n_sets; ++k)
        if (ms_set[k] < 0.97 * ms_set[0] && ms_set[k] < best_all) { best_all = ms_set[k]; best_set = k; }
    for (int q = 0; q < 4; ++q) b->s_k[q] = cand_set[best_set][q];
    b->timing = timing;
    if (ms_per_call) *ms_per_call = (float) best_all;
    return gnuais_batch_reset(b);
}

int gnuais_batch_sync(gnuais_batch *b)
{
    if (!b) return fail(GNUAIS_E_ARG, "sync: NULL batch");
    if (int rc = set_device(b)) return rc;
    HIP_TRY(hipStreamSynchronize(b->last[CHAIN].s));
    for (auto &st : b->s_k) HIP_TRY(hipStreamSynchronize(st));
    return GNUAIS_OK;
}


int gnuais_batch_filter(gnuais_batch *b, const int16_t *d_samples, int len, float *d_out,
                        void *stream)
{
    if (!b || !d_samples || !d_out) return fail(GNUAIS_E_ARG, "filter: NULL argument");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "filter: len out of range");
    if (int rc = set_device(b)) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (int rc = gnuais_batch_sync(b)) return rc;       // the sign-word scratch is shared
    if (int rc = run_fir(b, d_samples, len, d_out, s, (int) (b->calls % (unsigned) b->nbuf))) return rc;
    b->last[CHAIN].s = s;
    b->timed_last = false;
    return GNUAIS_OK;
}

// filter_run_buf() from and to HOST memory, for plain-C callers (gnuais_amd/csrc/protodec_hip.c: the reference's
// filter.h names): h_samples int16 [len][n_channels], h_out float [len][n_channels]; synchronous
int gnuais_batch_filter_host(gnuais_batch *b, const int16_t *h_samples, int len, float *h_out)
{
    if (!b || !h_samples || !h_out) return fail(GNUAIS_E_ARG, "filter_host: NULL argument");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "filter_host: len out of range");
    if (int rc = set_device(b)) return rc;
    const size_t n = (size_t) len * (size_t) b->N;
    HIP_TRY(b->stage_x.grow(n * sizeof(int16_t)));
    HIP_TRY(b->stage_f.grow(n * sizeof(float)));
    HIP_TRY(hipMemcpy(b->stage_x, h_samples, n * sizeof(int16_t), hipMemcpyHostToDevice));
    if (int rc = gnuais_batch_filter(b, b->stage_x, len, b->stage_f, nullptr)) return rc;
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipMemcpy(h_out, b->stage_f, n * sizeof(float), hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

int gnuais_batch_decode_bits(gnuais_batch *b, const uint8_t *h_bits, int stride,
                             const int32_t *h_count)
{
    if (!b || !h_bits || !h_count || stride <= 0) return fail(GNUAIS_E_ARG, "decode_bits: argument");
    if (int rc = gnuais_batch_sync(b)) return rc;
    b->clock_fresh = false;
    const int N = b->N, segcap = b->seg_words * 32, chunk = segcap * b->n_seg;
    int maxc = 0;
    for (int c = 0; c < N; ++c) {
        if (h_count[c] < 0 || h_count[c] > stride) return fail(GNUAIS_E_ARG, "decode_bits: count");
        maxc = std::max(maxc, h_count[c]);
    }
    const size_t rowlen = (size_t) b->n_seg * PACK_STRIDE;
    std::vector<uint32_t> words(rowlen * N), cnt((size_t) b->n_seg * N);
    for (int pos = 0; pos < maxc; pos += chunk) {
        std::fill(words.begin(), words.end(), 0u);
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (int c = 0; c < N; ++c) {
            const int n = std::max(0, std::min(chunk, h_count[c] - pos));
            const uint8_t *src = h_bits + (size_t) c * stride + pos;
            for (int k = 0; k < n; ++k) {
                const int seg = k / segcap, kk = k % segcap;
                if (src[k] & 1)
                    words[(size_t) c * rowlen + (size_t) seg * PACK_STRIDE + (kk >> 5)] |= 1u << (kk & 31);
            }
            for (int seg = 0; seg * segcap < n; ++seg)
                cnt[(size_t) c * b->n_seg + seg] = (uint32_t) std::min(segcap, n - seg * segcap);
        }
        HIP_TRY(hipMemcpy(b->segbits[0], words.data(), words.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->segcnt[0], cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
        HdlcLaunch h;
        fill_hdlc(b, h, 0);
        if (int rc = run_deframer(b, h, nullptr)) return rc;
        HIP_TRY(launch_hdlc_crc(h, nullptr));
        if (b->repair) HIP_TRY(launch_hdlc_repair(fill_repair(b, h), nullptr));
        if (b->frame_times) HIP_TRY(launch_frame_times(fill_frame_times(b, h, 0), nullptr));   // bits without samples: -1
        if (b->frame_signal) HIP_TRY(launch_frame_signal(fill_frame_signal(b, h, 0), nullptr));   // and (0, 0, 0)
        if (b->long_frames)                                                                        // D' on the same packs: t = -1
            if (int rc = run_long(b, h, 0, nullptr)) return rc;
        if (b->long_frames && b->long_frame_signal)                                                // their records: (0, 0, 0)
            HIP_TRY(launch_long_signal(long_signal_launch(b, 0), nullptr));
        if (b->streaming) b->ring_runs[b->ring_cur]++;
        b->hdlc_calls++;
        HIP_TRY(hipDeviceSynchronize());
    }
    b->last[CHAIN].s = nullptr;
    return GNUAIS_OK;
}

int gnuais_batch_last_bits(gnuais_batch *b, uint8_t *h_bits, int stride, int32_t *h_count)
{
    if (!b || !h_bits || !h_count || stride <= 0) return fail(GNUAIS_E_ARG, "last_bits: argument");
    if (int rc = gnuais_batch_sync(b)) return rc;
    const int N = b->N;
    const size_t rowlen = (size_t) b->n_seg * PACK_STRIDE;
    std::vector<uint32_t> words(rowlen * N), cnt((size_t) b->n_seg * N);
    HIP_TRY(hipMemcpy(words.data(), b->segbits[b->last_k], words.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cnt.data(), b->segcnt[b->last_k], cnt.size() * 4, hipMemcpyDeviceToHost));
    const int nseg_used = ((b->last_len + 31) / 32 + SEG_WORDS - 1) / SEG_WORDS;
    for (int c = 0; c < N; ++c) {
        int n = 0;
        uint8_t *dst = h_bits + (size_t) c * stride;
        for (int seg = 0; seg < nseg_used; ++seg) {
            const int m = (int) std::min<uint32_t>(cnt[(size_t) c * b->n_seg + seg],
                                                   (uint32_t) b->seg_words * 32);
            if (n + m > stride) return fail(GNUAIS_E_ARG, "last_bits: stride too small");
            const uint32_t *w = &words[(size_t) c * rowlen + (size_t) seg * PACK_STRIDE];
            for (int k = 0; k < m; ++k) dst[n + k] = (w[k >> 5] >> (k & 31)) & 1u;
            n += m;
        }
        h_count[c] = n;
    }
    return GNUAIS_OK;
}


int gnuais_batch_counters(gnuais_batch *b, gnuais_counters *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "counters: argument");
    const int N = b->N;
    std::vector<int32_t> v;
    if (int rc = read_out(b, b->counters, (size_t) N * 3, v)) return rc;
    for (int c = 0; c < N; ++c) {
        h_out[c].receivedframes = v[c];
        h_out[c].lostframes = v[(size_t) N + c];
        h_out[c].lostframes2 = v[(size_t) 2 * N + c];
    }
    return GNUAIS_OK;
}

int gnuais_batch_total_received(gnuais_batch *b, long long *total)
{
    if (!b || !total) return fail(GNUAIS_E_ARG, "total_received: argument");
    std::vector<int32_t> v;
    if (int rc = read_out(b, b->counters, (size_t) b->N, v)) return rc;
    long long t = 0;
    for (int32_t x : v) t += x;
    *total = t;
    return GNUAIS_OK;
}

int gnuais_batch_maxval(gnuais_batch *b, int16_t *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "maxval: argument");
    std::vector<int> v;
    if (int rc = read_out(b, b->maxval[b->max_last], (size_t) b->N, v)) return rc;
    for (int c = 0; c < b->N; ++c) h_out[c] = (int16_t) v[c];
    return GNUAIS_OK;
}

int gnuais_batch_pll_state(gnuais_batch *b, gnuais_pll_state *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "pll_state: argument");
    std::vector<uint32_t> v, lb, pv;
    if (int rc = read_out(b, b->pll, (size_t) b->N, v)) return rc;
    if (int rc = read_out(b, b->lastbit, (size_t) b->N, lb)) return rc;
    if (int rc = read_out(b, b->prev, (size_t) b->N, pv)) return rc;
    for (int c = 0; c < b->N; ++c) {
        h_out[c].pll = v[c] & 0xffffu;
        h_out[c].prev = pv[c] & 1;
        h_out[c].lastbit = lb[c] & 1;
    }
    return GNUAIS_OK;
}

int gnuais_batch_fsm_state(gnuais_batch *b, gnuais_fsm_state *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "fsm_state: argument");
    std::vector<uint32_t> v;
    if (int rc = read_out(b, b->ctl, (size_t) b->N, v)) return rc;
    for (int c = 0; c < b->N; ++c) {
        const uint32_t w = v[c];
        h_out[c].state = w & 7;
        h_out[c].nstartsign = (w >> 3) & 15;
        h_out[c].antallpreamble = (w >> 7) & 15;
        h_out[c].antallenner = (w >> 11) & 7;
        h_out[c].bitstuff = (w >> 14) & 1;
        h_out[c].last = (w >> 15) & 1;
        h_out[c].bufferpos = (w >> 16) & 511;
    }
    return GNUAIS_OK;
}

// protodec_reset() (protodec.c:87-100) for every receiver's decoder: the machine back to ST_SKURR with its counts
// cleared, a frame in progress dropped; receivedframes / lostframes / lostframes2 stay, as in the reference
int gnuais_batch_protodec_reset(gnuais_batch *b)
{
    if (!b) return fail(GNUAIS_E_ARG, "protodec_reset: NULL batch");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(launch_hdlc_fsm_reset(b->ctl, b->N, nullptr));
    if (int rc = long_zero_state(b, false)) return rc;      // D' likewise: its machine, not its counters or its ring
    HIP_TRY(hipStreamSynchronize(nullptr));
    return GNUAIS_OK;
}

// d->buffer (protodec.h:52, written at protodec.c:1019): the stored bits -- one per byte, stuffed 0s dropped -- of the
// frame a channel's decoder is in (ST_DATA / ST_STOPSIGN) or, between frames, of the last frame that reached its stop
// bit; *n_bits = -1 when neither is on record (no frame yet, or the last one was given up at 449 bits).  Rebuilt on the host from
// the candidate record the deframer keeps (raw bits incl. stuffing) and its partial word.
int gnuais_batch_frame_bits(gnuais_batch *b, int channel, uint8_t *h_bits, int cap, int *n_bits)
{
    if (!b || !h_bits || !n_bits || channel < 0 || channel >= b->N || cap < 0)
        return fail(GNUAIS_E_ARG, "frame_bits: argument");
    if (int rc = gnuais_batch_sync(b)) return rc;
    uint32_t w[HDLC_CTL_WORDS];
    for (int q = 0; q < HDLC_CTL_WORDS; ++q)
        HIP_TRY(hipMemcpy(&w[q], b->ctl + (size_t) q * (size_t) b->N + channel, 4, hipMemcpyDeviceToHost));
    *n_bits = -1;
    const uint32_t state = w[0] & 7, nstart = w[3];
    if (nstart == 0) return GNUAIS_OK;
    uint32_t rec[CAND_WORDS];
    HIP_TRY(hipMemcpy(rec, b->cand + ((size_t) channel * b->cand_K + (nstart - 1) % (uint32_t) b->cand_K) * CAND_WORDS,
                      sizeof rec, hipMemcpyDeviceToHost));
    int rawlen;
    const bool open = state == 4 || state == 5;             // ST_DATA, ST_STOPSIGN (protodec.h:33-34)
    if (open) {
        rawlen = (int) w[4];
        if ((rawlen >> 5) < CAND_WORDS - CAND_HDR) rec[CAND_HDR + (rawlen >> 5)] = w[1];   // the word being filled
    } else if (rec[0] >> 17) {                              // closed with a stop bit, good (CAND_VALID) or bad: its length is on record
        rawlen = (int) ((rec[0] >> 17) & 0x3ffu);
    } else {
        return GNUAIS_OK;                                   // given up at 449 bits (protodec.c:1024-1026), or overwritten
    }
    if (rawlen < 0 || rawlen > 32 * (CAND_WORDS - CAND_HDR)) return fail(GNUAIS_E_STATE, "frame_bits: record length");
    int n = 0, ones = 0;
    for (int i = 0; i < rawlen; ++i) {
        const uint8_t x = (rec[CAND_HDR + (i >> 5)] >> (i & 31)) & 1u;
        if (ones == 5) { ones = 0; continue; }              // the 0 after five 1s: protodec.c:1002-1006
        if (n < cap) h_bits[n] = x;
        ++n;
        ones = x ? ones + 1 : 0;
    }
    *n_bits = n;
    return GNUAIS_OK;
}

int gnuais_batch_history(gnuais_batch *b, int16_t *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "history: argument");
    const int N = b->N, NT = b->NT;
    std::vector<int16_t> v;
    if (int rc = read_out(b, b->hist[b->hist_cur], (size_t) N * NT, v)) return rc;
    for (int c = 0; c < N; ++c)
        for (int k = 0; k < NT; ++k) h_out[(size_t) c * NT + k] = v[(size_t) k * N + c];
    return GNUAIS_OK;
}

int gnuais_batch_last_signs(gnuais_batch *b, uint8_t *h_out, int stride)
{
    if (!b || !h_out || stride < b->last_len) return fail(GNUAIS_E_ARG, "last_signs: argument");
    if (int rc = gnuais_batch_sync(b)) return rc;
    const int N = b->N, W = (b->last_len + 31) / 32;
    std::vector<uint32_t> w(sgn_words_alloc(W, N));
    if (W) HIP_TRY(hipMemcpy(w.data(), b->sgn[b->last_k], w.size() * 4, hipMemcpyDeviceToHost));
    for (int c = 0; c < N; ++c)
        for (int n = 0; n < b->last_len; ++n)
            h_out[(size_t) c * stride + n] = (w[sgn_index(n >> 5, N, c)] >> (31 - (n & 31))) & 1u;
    return GNUAIS_OK;
}

// The long ring holds one launch's worst case: a long burst is 24 training bits, two flags and more than 426 + 16 frame
// bits, about 470 bits, over the most bits one deframer launch can be handed (as for the candidate ring in create), on
// every channel at once.  It is drained far more rarely than it could fill only if every channel sent nothing else.
static int long_ring_capacity(const gnuais_batch *b)
{
    const uint64_t launch_bits = std::max((uint64_t) b->bits_words * 32, (uint64_t) b->seg_words * 32 * (uint64_t) b->n_seg);
    return (int) std::max<uint64_t>(256, (uint64_t) b->N * (launch_bits / 470 + 2));
}

int gnuais_batch_info(const gnuais_batch *b, const char *name, double *value)
{
    if (!b || !name || !value) return fail(GNUAIS_E_ARG, "info: argument");
    // what the options select for the batch's table: the function plan_fir() starts from (fir_plan.cpp), nothing restated here
    const SignChoice c = sign_choice(b->sign, b->fir, b->N);
    if (!strcmp(name, "sign_exact")) *value = c.exact;
    else if (!strcmp(name, "sign_eps")) *value = c.eps;          // of the kernel the options select; FL2: the power of two it works with
    else if (!strcmp(name, "sign_flag_scale")) *value = c.th.fscale;
    else if (!strcmp(name, "sign_eps_seen")) *value = c.th.eps_seen;
    else if (!strcmp(name, "sign_eps_ahead")) *value = c.th.eps_ahead;
    else if (!strcmp(name, "sign_matrix_pipe")) *value = c.matrix_pipe;     // eligible: a call takes the matrix pipe when its length allows
    else if (!strcmp(name, "sign_central_taps")) *value = c.th.NC;
    else if (!strcmp(name, "first_effective_tap")) *value = b->k0;
    else if (!strcmp(name, "n_effective_taps")) *value = b->NE;
    else if (!strcmp(name, "compute_units")) *value = b->n_cu;
    else if (!strcmp(name, "device")) *value = b->device;
    else if (!strcmp(name, "afc_window")) *value = b->afc_W;
    else if (!strcmp(name, "segments")) *value = b->n_seg;
    else if (!strcmp(name, "pack_bits")) *value = b->seg_words * 32;        // bits a segment's pack holds; decode_bits fills packs to this
    else if (!strcmp(name, "frame_times")) *value = b->frame_times;
    else if (!strcmp(name, "frame_signal")) *value = b->frame_signal;
    else if (!strcmp(name, "occupancy")) *value = b->occ_E;
    else if (!strcmp(name, "rows")) *value = (double) b->rows;
    else if (!strcmp(name, "pll_form")) *value = b->pll_form;
    else if (!strcmp(name, "repair")) *value = b->repair;
    else if (!strcmp(name, "long_frames")) *value = b->long_frames;
    else if (!strcmp(name, "long_frame_cap")) *value = b->long_cap ? b->long_cap : long_ring_capacity(b);
    else if (!strcmp(name, "long_repair")) *value = b->long_repair;
    else if (!strcmp(name, "long_frame_signal")) *value = b->long_frame_signal;
    else if (!strcmp(name, "occupancy_lag"))    // LAG in rows: of the rings in use, else of the next gnuais_batch_occupancy switch
        *value = (double) occ_lag_rows(b->pllinc, b->NT, b->afc_W,
                                       (b->occ_E ? b->occ_long : b->long_frame_signal) ? FS_LONG_MAX_NBITS : FS_MAX_NBITS);
    else if (!strcmp(name, "long_cand_cap")) *value = b->long_cand_cap ? b->long_cand_cap : long_ring_capacity(b);
    else if (!strcmp(name, "unique")) *value = b->uq.window;
    else if (!strcmp(name, "unique_late")) *value = (double) b->uq.late;
    else if (!strcmp(name, "long_unique")) *value = b->lq.window;
    else if (!strcmp(name, "long_unique_late")) *value = (double) b->lq.late;
    else if (!strncmp(name, "stream_of_stage_", 16) && name[16] >= '0' && name[16] <= '3' && !name[17]) {
        // which of the batch's POOL candidate streams (creation order) serves stage 0 K2, 1 spare, 2 K2b, 3 K3 right now
        *value = -1;
        for (int q = 0; q < gnuais_batch::POOL; ++q)
            if (b->pool[q] == b->s_k[name[16] - '0']) *value = q;
    }
    else if (!strcmp(name, "stream_depth")) *value = gnuais_batch::NRING - 1;
    else return fail(GNUAIS_E_ARG, "info: unknown name");
    return GNUAIS_OK;
}

// The frames' receive times on / off (definition in include/gnuais_hip.h).  Synchronises: no call is in flight when the
// switch turns, so every K3 either has its timing launch behind it or has not.  What the ring holds when the feature
// comes on was appended without one: the whole array starts at -1.
int gnuais_batch_frame_times(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "frame_times: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "frame_times: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (!on && b->uq.window)
        return fail(GNUAIS_E_STATE, "frame_times: the batch merges duplicates by their times (gnuais_batch_unique); "
                                    "gnuais_batch_unique(b, 0) first");
    if (!on && b->frame_signal)
        return fail(GNUAIS_E_STATE, "frame_times: the batch finds its frames' spans by their times (gnuais_batch_frame_signal); "
                                    "gnuais_batch_frame_signal(b, 0) first");
    if (int rc = gnuais_batch_sync(b)) return rc;
    if (on && !b->frame_times) {
        HIP_TRY(b->times.ensure(sizeof(int64_t) * (size_t) b->frame_cap));
        HIP_TRY(hipMemset(b->times, 0xff, sizeof(int64_t) * (size_t) b->frame_cap));
    }
    b->frame_times = on != 0;
    return GNUAIS_OK;
}

// Messages of three to five slots on / off (definition in include/gnuais_hip.h).  Synchronises: no call is in flight when
// the switch turns, so every K3 either has D''s launch behind it or has not.  Either way D' starts afresh: its machine,
// its ring and its counters; its bit count is the chain's deframer's and needs nothing.
int gnuais_batch_long_frames(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "long_frames: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "long_frames: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (on && !b->long_ctl) {
        const size_t N = (size_t) b->N;
        b->long_cap = long_ring_capacity(b);
        HIP_TRY(b->long_open.ensure(sizeof(uint32_t) * N * LONG_REC_WORDS, true));
        HIP_TRY(b->long_counters.ensure(sizeof(int32_t) * N * 3, true));
        HIP_TRY(b->long_count.ensure(sizeof(uint32_t) * 2, true));
        HIP_TRY(b->long_ring.ensure(sizeof(gnuais_long_frame) * (size_t) b->long_cap));
        HIP_TRY(b->long_ctl.ensure(sizeof(uint32_t) * N * LONG_CTL_WORDS, true));    // last: long_zero_state() goes by it
    }
    if (int rc = long_zero_state(b, true)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    b->long_frames = on != 0;
    if (!on) b->long_repair = false;            // gnuais_batch_long_repair: nothing to repair without D'
    if (!on) b->long_frame_signal = false;      // gnuais_batch_long_frame_signal: nothing to measure either
    if (!on) b->lq.window = 0;                  // gnuais_batch_long_unique: nothing to merge either
    b->lq.n_tail = 0;                           // any switch: the ring starts over, and so do the merge's tail and late count
    b->lq.late = 0;
    return GNUAIS_OK;
}

// The repair of the long frames D' counts in `failed`, on / off (definition in include/gnuais_hip.h).  Synchronises: no
// call is in flight when the switch turns, so every D' launch is of the form the switch says and either has its repair
// launch behind it or has not.  D' itself is not reset: a frame in progress keeps its raw bits in `open` in either form.
// The candidate ring holds what one call's D' can close -- the long ring's own bound (long_ring_capacity) -- and the
// repair launch of the same call consumes it, so it cannot overflow across calls.
int gnuais_batch_long_repair(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "long_repair: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "long_repair: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (!b->long_frames)
        return fail(GNUAIS_E_STATE, "long_repair: the batch does not decode long frames (gnuais_batch_long_frames): "
                                    "the repair works on what that decoder counts as failed");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (on && !b->long_cand) {
        const size_t N = (size_t) b->N;
        b->long_cand_cap = b->long_cap;
        HIP_TRY(b->long_clean.ensure(sizeof(uint32_t) * N * LONG_REC_WORDS, true));
        HIP_TRY(b->long_cand_count.ensure(sizeof(uint32_t) * 2, true));
        HIP_TRY(b->long_cand.ensure(sizeof(uint32_t) * (size_t) b->long_cand_cap * LONG_CAND_WORDS));
    }
    if (on) {
        HIP_TRY(hipMemset(b->long_cand_count, 0, sizeof(uint32_t) * 2));
        b->long_parity = 0;
    }
    b->long_repair = on != 0;
    return GNUAIS_OK;
}

int gnuais_batch_long_repaired(gnuais_batch *b, int32_t *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "long_repaired: argument");
    if (!b->long_ctl) return fail(GNUAIS_E_STATE, "long_repaired: the batch has never decoded long frames (gnuais_batch_long_frames)");
    std::vector<int32_t> v;
    if (int rc = read_out(b, b->long_counters, (size_t) b->N * 3, v)) return rc;
    memcpy(h_out, v.data() + 2 * (size_t) b->N, sizeof(int32_t) * (size_t) b->N);
    return GNUAIS_OK;
}

static_assert(sizeof(gnuais_long_frame) == 152 && sizeof(gnuais_long_frame) == 4 * LONG_FRAME_WORDS, "gnuais_long_frame layout");

int gnuais_batch_pending_long_frames(gnuais_batch *b, int *n_out)
{
    if (!b || !n_out) return fail(GNUAIS_E_ARG, "pending_long_frames: argument");
    uint32_t have = 0;
    bool overflow = false;
    if (int rc = long_pending(b, "pending_long_frames", have, overflow)) return rc;
    *n_out = (int) have;
    return GNUAIS_OK;
}

// Everything queued, consumed once, in (channel, 37-bit stamp) order.  Long frames are rare -- the ring holds a handful
// per drain -- so the records cross PCIe as the kernel appended them and are put in order here.
// h_signal: entry for entry, the records of gnuais_batch_long_frame_signal as well, through the sort's own permutation
static int drain_long_impl(gnuais_batch *b, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max, int *n_out,
                           const char *who)
{
    const std::string name(who);
    *n_out = 0;
    uint32_t have = 0;
    bool overflow = false;
    if (int rc = long_pending(b, who, have, overflow)) return rc;
    if ((uint32_t) max < have) return fail(GNUAIS_E_ARG, (name + ": frame buffer too small").c_str());
    if (have) {
        std::vector<gnuais_long_frame> v(have);
        std::vector<gnuais_frame_signal> sig(h_signal ? have : 0);
        HIP_TRY(hipMemcpy(v.data(), b->long_ring, sizeof(gnuais_long_frame) * have, hipMemcpyDeviceToHost));
        if (h_signal) HIP_TRY(hipMemcpy(sig.data(), b->long_signal, sizeof(gnuais_frame_signal) * have, hipMemcpyDeviceToHost));
        const auto stamp = [](const gnuais_long_frame &f) { return (uint64_t) f.end_bit | ((uint64_t) ((f.flags >> 1) & 31) << 32); };
        std::vector<uint32_t> order(have);
        for (uint32_t i = 0; i < have; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) {
            const gnuais_long_frame &x = v[i], &y = v[j];
            return x.channel != y.channel ? x.channel < y.channel : stamp(x) < stamp(y);
        });
        for (uint32_t i = 0; i < have; ++i) {
            h_out[i] = v[order[i]];
            if (h_signal) h_signal[i] = sig[order[i]];
        }
    }
    *n_out = (int) have;
    HIP_TRY(hipMemset(b->long_count, 0, sizeof(uint32_t) * 2));
    if (overflow) return fail(GNUAIS_E_OVERFLOW, (name + ": long-frame ring overflowed, frames were dropped").c_str());
    return GNUAIS_OK;
}

int gnuais_batch_drain_long_frames(gnuais_batch *b, gnuais_long_frame *h_out, int max, int *n_out)
{
    if (!b || !n_out || max < 0 || (max && !h_out)) return fail(GNUAIS_E_ARG, "drain_long_frames: argument");
    return drain_long_impl(b, h_out, nullptr, max, n_out, "drain_long_frames");
}

// the same with, entry for entry, their power and carrier error (gnuais_batch_long_frame_signal)
int gnuais_batch_drain_long_frames_signal(gnuais_batch *b, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max,
                                          int *n_out)
{
    if (!b || !n_out || max < 0 || (max && (!h_out || !h_signal))) return fail(GNUAIS_E_ARG, "drain_long_frames_signal: argument");
    *n_out = 0;
    if (!b->long_frame_signal)
        return fail(GNUAIS_E_STATE, "drain_long_frames_signal: the batch does not measure its long frames (gnuais_batch_long_frame_signal)");
    static gnuais_frame_signal none_s;
    return drain_long_impl(b, h_out, h_signal ? h_signal : &none_s, max, n_out, "drain_long_frames_signal");
}

int gnuais_batch_long_counters(gnuais_batch *b, int32_t *h_delivered, int32_t *h_failed)
{
    if (!b || !h_delivered || !h_failed) return fail(GNUAIS_E_ARG, "long_counters: argument");
    if (!b->long_ctl) return fail(GNUAIS_E_STATE, "long_counters: the batch has never decoded long frames (gnuais_batch_long_frames)");
    std::vector<int32_t> v;
    if (int rc = read_out(b, b->long_counters, (size_t) b->N * 2, v)) return rc;
    memcpy(h_delivered, v.data(), sizeof(int32_t) * (size_t) b->N);
    memcpy(h_failed, v.data() + b->N, sizeof(int32_t) * (size_t) b->N);
    return GNUAIS_OK;
}

int gnuais_batch_long_fsm_state(gnuais_batch *b, gnuais_fsm_state *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "long_fsm_state: argument");
    if (!b->long_ctl) return fail(GNUAIS_E_STATE, "long_fsm_state: the batch has never decoded long frames (gnuais_batch_long_frames)");
    std::vector<uint32_t> v;
    if (int rc = read_out(b, b->long_ctl, (size_t) b->N, v)) return rc;
    for (int c = 0; c < b->N; ++c) {
        const uint32_t w = v[c];
        h_out[c].state = w & 7;
        h_out[c].nstartsign = (w >> 3) & 15;
        h_out[c].antallpreamble = (w >> 7) & 15;
        h_out[c].antallenner = (w >> 11) & 7;
        h_out[c].bitstuff = (w >> 14) & 1;
        h_out[c].last = (w >> 15) & 1;
        h_out[c].bufferpos = (w >> 16) & 2047;
    }
    return GNUAIS_OK;
}

// The repair of CRC-failed candidates on / off (definition in include/gnuais_hip.h).  Synchronises: no call is in flight
// when the switch turns, so every K3 either has its repair launch behind it or has not.
int gnuais_batch_repair(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "repair: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "repair: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (int rc = gnuais_batch_sync(b)) return rc;
    if (on) HIP_TRY(b->repaired.ensure(sizeof(int32_t) * (size_t) b->N, true));
    b->repair = on != 0;
    return GNUAIS_OK;
}

// The duplicate merge on / off (definition in include/gnuais_hip.h).  Nothing runs per call, so the switch only sets
// the window and empties the carried state; it synchronises like the other switches.
int gnuais_batch_unique(gnuais_batch *b, int window_rows)
{
    if (!b || window_rows < 0) return fail(GNUAIS_E_ARG, "unique: NULL batch or a negative window");
    if (b->streaming) return fail(GNUAIS_E_STATE, "unique: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (window_rows && !b->frame_times)
        return fail(GNUAIS_E_STATE, "unique: the batch does not time its frames (gnuais_batch_frame_times): copies are "
                                    "merged by their receive times");
    if (int rc = gnuais_batch_sync(b)) return rc;
    b->uq.window = window_rows;
    b->uq.n_tail = 0;
    b->uq.late = 0;
    return GNUAIS_OK;
}

// The duplicate merge of the long frames on / off (definition in include/gnuais_hip.h).  Like gnuais_batch_unique: the
// switch sets the window and empties the carried state -- a tail and a late count of its own.
int gnuais_batch_long_unique(gnuais_batch *b, int window_rows)
{
    if (!b || window_rows < 0) return fail(GNUAIS_E_ARG, "long_unique: NULL batch or a negative window");
    if (!b->long_frames)
        return fail(GNUAIS_E_STATE, "long_unique: the batch does not decode long frames (gnuais_batch_long_frames): "
                                    "the merge works on that decoder's records");
    if (int rc = gnuais_batch_sync(b)) return rc;
    b->lq.window = window_rows;
    b->lq.n_tail = 0;
    b->lq.late = 0;
    return GNUAIS_OK;
}

int gnuais_batch_long_unique_late(gnuais_batch *b, long long *late)
{
    if (!b || !late) return fail(GNUAIS_E_ARG, "long_unique_late: argument");
    *late = b->lq.late;
    return GNUAIS_OK;
}

int gnuais_batch_unique_late(gnuais_batch *b, long long *late)
{
    if (!b || !late) return fail(GNUAIS_E_ARG, "unique_late: argument");
    *late = b->uq.late;
    return GNUAIS_OK;
}

int gnuais_batch_repaired(gnuais_batch *b, int32_t *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "repaired: argument");
    if (!b->repaired) {                         // never switched on: nothing repaired
        if (int rc = gnuais_batch_sync(b)) return rc;
        std::fill(h_out, h_out + b->N, 0);
        return GNUAIS_OK;
    }
    std::vector<int32_t> v;
    if (int rc = read_out(b, b->repaired, (size_t) b->N, v)) return rc;
    std::copy(v.begin(), v.end(), h_out);
    return GNUAIS_OK;
}

// input sample index = t * mul + off, for the batch's configuration as it is now: the nominal decision instant
int gnuais_batch_time_map(const gnuais_batch *b, int kind, long long *mul, long long *off)
{
    if (!b || !mul || !off) return fail(GNUAIS_E_ARG, "time_map: argument");
    const long long d_f = (b->NT + 1) / 2, half_w = b->afc_W / 2;
    switch (kind) {
    case GNUAIS_INPUT_AUDIO:
        *mul = 1;
        *off = -d_f;
        return GNUAIS_OK;
    case GNUAIS_INPUT_IQ:
        *mul = 1;
        *off = -d_f - half_w;
        return GNUAIS_OK;
    case GNUAIS_INPUT_WIDEBAND: {
        if (!b->wide.K) return fail(GNUAIS_E_STATE, "time_map: no channeliser configured (gnuais_batch_channeliser)");
        if (b->wide.U > 1)
            return fail(GNUAIS_E_STATE, "time_map: the wide stage resamples by a ratio up / down with up > 1: use "
                                        "gnuais_batch_time_map_ratio");
        const long long D = b->wide.D, T = b->wide.T;
        *mul = D;
        *off = (-d_f - half_w) * D + D - 1 - (T - 1) / 2;
        return GNUAIS_OK;
    }
    default:
        return fail(GNUAIS_E_ARG, "time_map: kind must be GNUAIS_INPUT_AUDIO, _IQ or _WIDEBAND");
    }
}

// input sample index = floor((t * num + off) / den): gnuais_batch_time_map with the rational channeliser's ratio
int gnuais_batch_time_map_ratio(const gnuais_batch *b, int kind, long long *num, long long *den, long long *off)
{
    if (!b || !num || !den || !off) return fail(GNUAIS_E_ARG, "time_map_ratio: argument");
    if (kind != GNUAIS_INPUT_WIDEBAND || !b->wide.K || b->wide.U == 1) {      // den = 1: the integer map, with its checks
        *den = 1;
        return gnuais_batch_time_map(b, kind, num, off);
    }
    const long long d_f = (b->NT + 1) / 2, half_w = b->afc_W / 2, D = b->wide.D, T = b->wide.T;
    *num = D;
    *den = b->wide.U;
    *off = (-d_f - half_w) * D + D - 1 - (T - 1) / 2;
    return GNUAIS_OK;
}

int gnuais_batch_n_channels(const gnuais_batch *b) { return b ? b->N : 0; }
int gnuais_batch_n_taps(const gnuais_batch *b) { return b ? b->NT : 0; }

int gnuais_batch_set_timing(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "set_timing: NULL batch");
    b->timing = on != 0;
    if (on) b->timed_calls = 0;
    return GNUAIS_OK;
}

// ms[0] K1 fir_slice  [1] K2 pll  [2] K2b hdlc_deframe  [3] K3 hdlc_crc
// [4] first event to last event of the call
static int timing_of(gnuais_batch *b, unsigned long long call, float *ms)
{
    const Event *ev = b->evr[call % gnuais_batch::TIMING_RING];
    HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], ev[2], ev[6]));
    HIP_TRY(hipEventElapsedTime(&ms[2], ev[5], ev[7]));
    HIP_TRY(hipEventElapsedTime(&ms[3], ev[9], ev[4]));
    HIP_TRY(hipEventElapsedTime(&ms[4], ev[0], ev[4]));
    return GNUAIS_OK;
}

int gnuais_batch_last_timing(gnuais_batch *b, float *ms5)
{
    if (!b || !ms5) return fail(GNUAIS_E_ARG, "last_timing: argument");
    if (!b->timed_calls) return fail(GNUAIS_E_STATE, "last_timing: no timed run");
    if (int rc = gnuais_batch_sync(b)) return rc;
    return timing_of(b, b->timed_calls - 1, ms5);
}

int gnuais_batch_mean_timing(gnuais_batch *b, float *ms5, int *n_calls)
{
    if (!b || !ms5 || !n_calls) return fail(GNUAIS_E_ARG, "mean_timing: argument");
    if (!b->timed_calls) return fail(GNUAIS_E_STATE, "mean_timing: no timed run");
    if (int rc = gnuais_batch_sync(b)) return rc;
    const unsigned long long n = std::min<unsigned long long>(b->timed_calls, gnuais_batch::TIMING_RING);
    double acc[5] = {0, 0, 0, 0, 0};
    for (unsigned long long i = 0; i < n; ++i) {
        float t[5];
        if (int rc = timing_of(b, b->timed_calls - 1 - i, t)) return rc;
        for (int q = 0; q < 5; ++q) acc[q] += t[q];
    }
    for (int q = 0; q < 5; ++q) ms5[q] = (float) (acc[q] / (double) n);
    *n_calls = (int) n;
    return GNUAIS_OK;
}

int gnuais_crc16_batch(int device, const uint8_t *h_data, int stride, const int32_t *h_len,
                       int n_msgs, uint16_t *h_crc)
{
    if (!h_data || !h_len || !h_crc || stride <= 0 || n_msgs <= 0)
        return fail(GNUAIS_E_ARG, "crc16_batch: argument");
    HIP_TRY(hipSetDevice(device));
    Buf<uint8_t> d_data;
    Buf<int32_t> d_len;
    Buf<uint16_t> d_crc;
    hipError_t e = d_data.alloc((size_t) stride * n_msgs);
    if (e == hipSuccess) e = d_len.alloc(sizeof(int32_t) * n_msgs);
    if (e == hipSuccess) e = d_crc.alloc(sizeof(uint16_t) * n_msgs);
    if (e == hipSuccess) e = hipMemcpy(d_data, h_data, (size_t) stride * n_msgs, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_len, h_len, sizeof(int32_t) * n_msgs, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_crc16(d_data, stride, d_len, n_msgs, d_crc, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_crc, d_crc, sizeof(uint16_t) * n_msgs, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GNUAIS_E_HIP, "crc16_batch", e);
    return GNUAIS_OK;
}

int gnuais_crc16_bits(int device, const uint8_t *h_bits, int n_bytes, uint16_t *h_crc, uint8_t *h_msb, int n_out)
{
    if (!h_bits || !h_crc || n_bytes <= 0 || n_bytes > 64 || n_out < 0 || n_out > 8 * n_bytes || (n_out > 0 && !h_msb))
        return fail(GNUAIS_E_ARG, "crc16_bits: argument (1..64 bytes, n_out <= 8 * n_bytes)");
    HIP_TRY(hipSetDevice(device));
    // one allocation: [bits 512][msb 512][crc]
    Buf<uint8_t> d;
    hipError_t e = d.alloc(512 + 512 + 16);
    if (e == hipSuccess) e = hipMemcpy(d, h_bits, (size_t) n_bytes * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_crc16_bits(d, n_bytes, reinterpret_cast<uint16_t *>(d + 1024), n_out ? d + 512 : nullptr, n_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_crc, d + 1024, sizeof(uint16_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_out) e = hipMemcpy(h_msb, d + 512, (size_t) n_out, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GNUAIS_E_HIP, "crc16_bits", e);
    return GNUAIS_OK;
}

int gnuais_tile_channels(const int16_t *d_base, int n_base, int len, int16_t *d_out,
                         int n_channels, void *stream)
{
    if (!d_base || !d_out || n_base <= 0 || len <= 0 || n_channels <= 0)
        return fail(GNUAIS_E_ARG, "tile_channels: argument");
    HIP_TRY(launch_tile_channels(d_base, n_base, len, d_out, n_channels, (hipStream_t) stream));
    return GNUAIS_OK;
}

} // extern "C"
