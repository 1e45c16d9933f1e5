// capi_ingest.hip -- the C ABI's input side (include/gnuais_hip.h): the stages in front of the chain -- discriminator,
// carrier-error stage, channeliser with its host tables -- and the entries that take a form's input from device or
// host memory and hand the audio to gnuais_batch_run (gnuais_capi.hip).  Host code only.
#include "batch.h"
#include "frame_signal.h"
#include "occupancy.h"
#include "resample_plan.h"
#include "wide_format.h"

// fmt: the sample format of a wide column (GNUAIS_FMT_*); the narrowband forms are int16
static Form form(const gnuais_batch *b, FormId f, int fmt = GNUAIS_FMT_CS16)
{
    switch (f) {
    case AUDIO: return {2, b->N, 1, 1u << CHAIN};
    case IQ: return {4, b->N, 1, 1u << DISC | (b->afc_W ? 1u << AFC : 0u) | 1u << CHAIN};
    default: return {wide_format_bytes(fmt), b->wide.K ? b->N / b->wide.K : 0, b->wide.D, 1u << CHAN | form(b, IQ).stages,
                 b->wide.U};
    }
}

// An intermediate buffer of `bytes`, allocated on first use once the device has room for it: `what` of N x max_len
template <class T>
static int alloc_checked(gnuais_batch *b, Buf<T> &p, size_t bytes, const char *who, const char *what)
{
    if (p) return GNUAIS_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > free_b) {
        char msg[256];
        snprintf(msg, sizeof msg, "%s: %s for %d channels x %d samples needs %.2f GB of device memory, device %d has %.2f "
                 "GB free of %.2f", who, what, b->N, b->max_len, bytes / 1e9, b->device, free_b / 1e9, total_b / 1e9);
        return fail(GNUAIS_E_HIP, msg);
    }
    HIP_TRY(p.alloc(bytes));
    return GNUAIS_OK;
}

// a host table onto the device (none for an empty one)
template <class T>
static int to_device(Buf<T> &p, const std::vector<T> &v)
{
    if (v.empty()) return GNUAIS_OK;
    HIP_TRY(p.alloc(sizeof(T) * v.size()));
    HIP_TRY(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return GNUAIS_OK;
}

// the wide stage's carry and sample count (configuration kept)
int gnuais::chan_zero_state(gnuais_batch *b)
{
    WideStage &w = b->wide;
    if (w.K)
        for (auto &p : w.hist)
            if (p) HIP_TRY(hipMemset(p, 0, sizeof(uint32_t) * (size_t) w.H * (size_t) (b->N / w.K)));
    w.cur = 0;
    w.n = 0;
    b->last[CHAN].used = false;
    return GNUAIS_OK;
}

// the AFC stage's carry: row count, delay line, block sums (window kept)
int gnuais::afc_zero_state(gnuais_batch *b)
{
    if (b->afc_W) {
        const size_t N = (size_t) b->N;
        HIP_TRY(hipMemset(b->afc_delay, 0, sizeof(int16_t) * N * (size_t) (b->afc_W / 2)));
        HIP_TRY(hipMemset(b->afc_blk, 0, sizeof(int64_t) * 2 * N * (size_t) b->afc_nb));
    }
    b->afc_n = 0;
    b->afc_est_row = -1;
    b->last[AFC].used = false;
    return GNUAIS_OK;
}

// gnuais_batch_occupancy: the run starts anew at the current row, no epoch is final, the queue is empty (size kept)
int gnuais::occ_zero_state(gnuais_batch *b)
{
    if (b->occ_E && !b->occ_cover_clean)
        HIP_TRY(hipMemset(b->occ_cover, 0, (size_t) b->occ_CB * (size_t) b->N));
    b->occ_cover_clean = true;
    b->occ_v0 = b->rows;
    b->occ_next = 0;
    b->occ_seq = b->occ_drained = 0;
    b->occ_lost = 0;
    return GNUAIS_OK;
}

// the first whole block of the run the epochs are counted in
static long long occ_b0(const gnuais_batch *b) { return (long long) ((b->occ_v0 + FS_BLOCK - 1) / FS_BLOCK); }

// the longest frame that covers: the rings and LAG are those of the feature's state when occupancy was switched on
static int occ_max_nbits(const gnuais_batch *b) { return b->occ_long ? FS_LONG_MAX_NBITS : FS_MAX_NBITS; }
static_assert(FS_LONG_MAX_NBITS == GNUAIS_LONG_MAX_BITS, "the long span of the signal ring and of LAG");

int gnuais::occ_cover(gnuais_batch *b, const HdlcLaunch &h, int len, hipStream_t s)
{
    const size_t N = (size_t) b->N;
    const long long n0 = (long long) b->rows, b0 = occ_b0(b);
    // The first call of a run: whatever the run before it left in the cover ring goes, behind that run's last tail in
    // this stream's order.  (The code ring needs nothing: every block of an epoch is coded before the epoch is final.)
    if (b->rows == b->occ_v0 && !b->occ_cover_clean)
        HIP_TRY(hipMemsetAsync(b->occ_cover, 0, (size_t) b->occ_CB * N, s));
    b->occ_cover_clean = false;
    OccCoverLaunch c;
    c.frames = h.frames; c.frame_count = h.frame_count; c.frame_cap = h.frame_cap;
    c.times = b->times; c.cover = b->occ_cover;
    c.CB = b->occ_CB; c.N = b->N;
    c.len = len; c.n0 = n0;
    c.pllinc = b->pllinc; c.n_taps = b->NT; c.afc_window = b->afc_W;
    c.v0 = (int64_t) b->occ_v0; c.b0 = b0;
    HIP_TRY(launch_occ_cover(c, s));
    return GNUAIS_OK;
}

int gnuais::occ_finalise(gnuais_batch *b, int len, hipStream_t s)
{
    const size_t N = (size_t) b->N;
    const long long n0 = (long long) b->rows, b0 = occ_b0(b);
    // The epochs this call makes final: the host knows them from n0, len and v0 alone
    const long long lag = occ_lag_rows(b->pllinc, b->NT, b->afc_W, occ_max_nbits(b)), E = b->occ_E;
    while (n0 + len > FS_BLOCK * (b0 + (b->occ_next + 1) * E) - 1 + lag) {
        const int slot = (int) (b->occ_seq % OCC_RING_EPOCHS);
        OccEpochLaunch e;
        e.codes = b->occ_codes; e.cover = b->occ_cover; e.carry = b->occ_carry;
        e.out = b->occ_out.p + (size_t) slot * N;
        e.CB = b->occ_CB; e.N = b->N; e.E = b->occ_E; e.margin = b->occ_margin;
        e.first = b0 + b->occ_next * E;
        e.first_epoch = b->occ_next == 0;
        HIP_TRY(launch_occ_epoch(e, s));
        if (b->occ_seq - b->occ_drained == OCC_RING_EPOCHS) {       // the slot's epoch was never drained
            b->occ_drained++;
            b->occ_lost++;
        }
        b->occ_first[slot] = e.first;
        b->occ_seq++;
        b->occ_next++;
    }
    return GNUAIS_OK;
}

// the launch behind D' and the long repair of a call of len rows from row b->rows on (len <= 0: bits without samples).
// As for the chain's frames (fill_frame_signal), the records of a call that did not come through run_form get (0, 0, 0)
// -- v0 behind its last row -- and only a call that did has cover bytes to store.
LongSignalLaunch gnuais::long_signal_launch(const gnuais_batch *b, int len)
{
    LongSignalLaunch a;
    a.frames = b->long_ring.p; a.frame_count = b->long_count; a.frame_cap = (uint32_t) b->long_cap;
    a.ring = b->fs_ring; a.signal = b->long_signal.p;
    a.RB = b->fs_RB; a.N = b->N;
    a.len = len; a.n0 = (int64_t) b->rows;
    a.pllinc = b->pllinc; a.n_taps = b->NT; a.afc_window = b->afc_W;
    a.v0 = (int64_t) (b->fs_iq_call ? b->fs_v0 : b->rows + (unsigned long long) std::max(len, 0));
    if (b->occ_E && b->occ_long && b->fs_iq_call && len > 0) {
        a.cover = b->occ_cover; a.CB = b->occ_CB;
        a.occ_v0 = (int64_t) b->occ_v0; a.b0 = occ_b0(b);
    }
    return a;
}

extern "C" {

// ---- complex baseband in (include/gnuais_hip.h): the discriminator (iq_disc.hip) in front of the unchanged chain ----

// afc: the launch also takes the block sums of the rows from afc_n on (afc_launch follows on the same stream)
static int disc_launch(gnuais_batch *b, const int16_t *d_iq, int len, int16_t *d_out, hipStream_t s, bool afc = false)
{
    if (afc)
        HIP_TRY(launch_iq_discriminator_afc(d_iq, d_out, b->iq_prev, b->N, len, b->afc_blk, b->afc_nb, b->afc_n, s));
    else
        HIP_TRY(launch_iq_discriminator(d_iq, d_out, b->iq_prev, b->N, len, s));
    b->last[DISC] = {s, true};
    return GNUAIS_OK;
}

int gnuais_batch_discriminate(gnuais_batch *b, const int16_t *d_iq, int len, int16_t *d_out, void *stream)
{
    if (!b || !d_iq || !d_out) return fail(GNUAIS_E_ARG, "discriminate: NULL argument");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "discriminate: len out of range (max_len)");
    if (int rc = set_device(b)) return rc;
    if (int rc = drain(b, 1u << DISC, (hipStream_t) stream)) return rc;
    return disc_launch(b, d_iq, len, d_out, (hipStream_t) stream);
}

// ---- the carrier-error stage (include/gnuais_hip.h, afc.hip) between the discriminator and the chain ----

int gnuais_batch_afc(gnuais_batch *b, int window)
{
    if (!b) return fail(GNUAIS_E_ARG, "afc: NULL batch");
    if (window && (window < AFC_MIN_WINDOW || window > AFC_MAX_WINDOW || window % (2 * AFC_BLOCK)))
        return fail(GNUAIS_E_ARG, "afc: the window must be 0 (off) or a multiple of 128 from 128 to 16384");
    if (b->occ_E && window > b->occ_W)
        return fail(GNUAIS_E_STATE, "afc: the rings of gnuais_batch_occupancy are sized for the window it was switched on at; "
                                    "switch it off first");
    if (int rc = set_device(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(b->afc_blk.release());
    HIP_TRY(b->afc_delay.release());
    HIP_TRY(b->afc_est.release());
    b->afc_W = 0;
    if (window) {
        const size_t N = (size_t) b->N;
        const int call_blocks = (b->max_len + AFC_BLOCK - 1) / AFC_BLOCK + 1;      // a call that starts inside a block
        // the blocks of the oldest window a call reads up to the last one it writes
        b->afc_nb = window / AFC_BLOCK + call_blocks + 1;
        if (int rc = alloc_checked(b, b->afc_blk, sizeof(int64_t) * 2 * N * (size_t) b->afc_nb, "afc", "the block sums")) return rc;
        if (int rc = alloc_checked(b, b->afc_delay, sizeof(int16_t) * N * (size_t) (window / 2), "afc", "the delay line")) return rc;
        if (int rc = alloc_checked(b, b->afc_est, sizeof(int16_t) * N * (size_t) call_blocks, "afc", "the estimates")) return rc;
        b->afc_W = window;
    }
    if (int rc = afc_zero_state(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return GNUAIS_OK;
}

// behind disc_launch(.., afc = true) on s: the estimates of the blocks this call's output rows need, then the corrected
// audio of its len rows
static int afc_launch(gnuais_batch *b, const int16_t *d_audio, int len, int16_t *d_out, hipStream_t s)
{
    const unsigned long long n0 = b->afc_n, n1 = n0 + (unsigned long long) len, L = (unsigned long long) (b->afc_W / 2);
    long long j_lo = 0;
    if (n1 > L) {                                // row n1 - 1 has m >= 0: blocks (max(n0 - L, 0)) / 64 .. (n1 - 1 - L) / 64
        j_lo = (long long) ((n0 > L ? n0 - L : 0) / AFC_BLOCK);
        const int n_est = (int) ((long long) ((n1 - 1 - L) / AFC_BLOCK) - j_lo) + 1;
        HIP_TRY(launch_afc_estimate(b->afc_blk, b->afc_nb, b->N, b->afc_est, j_lo, n_est, b->afc_W, s));
        b->afc_est_row = n_est - 1;
    }
    HIP_TRY(launch_afc_apply(d_audio, b->afc_delay, b->afc_est, j_lo, d_out, b->N, len, b->afc_W, n0, s));
    b->afc_n = n1;
    b->last[AFC] = {s, true};
    return GNUAIS_OK;
}

int gnuais_batch_afc_apply(gnuais_batch *b, const int16_t *d_iq, int len, int16_t *d_out, void *stream)
{
    if (!b || !d_iq || !d_out) return fail(GNUAIS_E_ARG, "afc_apply: NULL argument");
    if (!b->afc_W) return fail(GNUAIS_E_STATE, "afc_apply: the AFC is off (gnuais_batch_afc)");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "afc_apply: len out of range (max_len)");
    if (int rc = set_device(b)) return rc;
    hipStream_t s = (hipStream_t) stream;
    if (int rc = drain(b, 1u << DISC | 1u << AFC, s)) return rc;
    if (int rc = alloc_checked(b, b->iq_audio, form(b, AUDIO).bytes_of(b->max_len), "afc_apply", "the discriminator's audio"))
        return rc;
    if (int rc = disc_launch(b, d_iq, len, b->iq_audio, s, true)) return rc;
    return afc_launch(b, b->iq_audio, len, d_out, s);
}

int gnuais_batch_afc_estimate(gnuais_batch *b, int16_t *h_out)
{
    if (!b || !h_out) return fail(GNUAIS_E_ARG, "afc_estimate: NULL argument");
    if (!b->afc_W) return fail(GNUAIS_E_STATE, "afc_estimate: the AFC is off (gnuais_batch_afc)");
    if (int rc = set_device(b)) return rc;
    if (b->afc_est_row < 0) {
        memset(h_out, 0, sizeof(int16_t) * (size_t) b->N);
        return GNUAIS_OK;
    }
    if (b->last[AFC].used) HIP_TRY(hipStreamSynchronize(b->last[AFC].s));
    HIP_TRY(hipMemcpy(h_out, b->afc_est + (size_t) b->afc_est_row * (size_t) b->N, sizeof(int16_t) * (size_t) b->N,
                      hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

// ---- wideband in (include/gnuais_hip.h): the wide stage (wide_kernels.h, planned by resample_plan.cpp) in front of the
// discriminator ----

static long long rnd_away(double x) { return lround(x); }

static long long gcd_ll(long long a, long long b)
{
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

// the period of offset f at rate R, or 0 if it exceeds 2^20
static int chan_period(int R, int f)
{
    const long long g = gcd_ll(std::llabs((long long) f), (long long) R);
    const long long P = (long long) R / g;
    return P > (1LL << 20) ? 0 : (int) P;
}

static void chan_mixer(int R, int f, int P, int16_t *cs)
{
    for (int p = 0; p < P; ++p) {
        long long q = ((long long) f * p) % R;
        if (q < 0) q += R;
        const double th = 2.0 * M_PI * (double) q / (double) R;
        cs[2 * p] = (int16_t) rnd_away(32767.0 * cos(th));
        cs[2 * p + 1] = (int16_t) rnd_away(32767.0 * sin(th));
    }
}

int gnuais_channeliser_default_taps(int decim, int16_t *out, int cap, int *n_taps)
{
    if (decim < 1 || decim > 64) return fail(GNUAIS_E_ARG, "channeliser_default_taps: decim must be 1..64");
    std::vector<int16_t> h;
    resample_default_taps(1, decim, h);
    const int T = (int) h.size();
    if (n_taps) *n_taps = T;
    if (!out) return GNUAIS_OK;
    if (cap < T) return fail(GNUAIS_E_ARG, "channeliser_default_taps: cap < 16*decim + 1");
    memcpy(out, h.data(), sizeof(int16_t) * (size_t) T);
    return GNUAIS_OK;
}

int gnuais_channeliser_mixer_table(int in_rate_hz, int offset_hz, int16_t *out, int cap, int *period)
{
    if (in_rate_hz <= 0) return fail(GNUAIS_E_ARG, "channeliser_mixer_table: in_rate_hz must be > 0");
    const int P = chan_period(in_rate_hz, offset_hz);
    if (!P) return fail(GNUAIS_E_ARG, "channeliser_mixer_table: the offset's mixer period R / gcd(|f|, R) exceeds 2^20");
    if (period) *period = P;
    if (!out) return GNUAIS_OK;
    if (cap < P) return fail(GNUAIS_E_ARG, "channeliser_mixer_table: cap < period");
    chan_mixer(in_rate_hz, offset_hz, P, out);
    return GNUAIS_OK;
}

// the checks of rate and offsets both entries share, in the name of the entry `who`: before the taps' checks
static int chan_shape_check(const gnuais_batch *b, const char *who, int in_rate_hz, int n_offsets)
{
    char msg[200];
    const char *what = nullptr;
    if (in_rate_hz <= 0) what = "in_rate_hz must be > 0";
    else if (n_offsets < 1 || n_offsets > CHAN_MAX_K) what = "n_offsets must be 1..32";
    else if (b->N % n_offsets) what = "the batch's channel count is not a multiple of n_offsets";
    if (what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return fail(GNUAIS_E_ARG, msg);
    }
    return GNUAIS_OK;
}

// Behind an entry's own checks of the ratio and of the prototype h, in the name of the entry `who`: the mixer periods'
// check, the mixer tables (C lo, S hi) and the plan (resample_plan.h; na: the fast form's accumulators for the entry's
// kernels, 0 = the direct form; `rational`: with the group table), then all of it onto the device (synchronises it);
// zeroes the carry and the sample count.  A failure behind the checks leaves the stage unconfigured.
static int wide_configure(gnuais_batch *b, const char *who, int up, int down, int in_rate_hz, const int32_t *offsets_hz,
                          int n_offsets, const std::vector<int16_t> &h, int na, bool rational)
{
    char msg[200];
    const int K = n_offsets, T = (int) h.size();
    int per[CHAN_MAX_K], off[CHAN_MAX_K], total = 0;
    for (int k = 0; k < K; ++k) {
        per[k] = chan_period(in_rate_hz, offsets_hz[k]);
        if (!per[k]) {
            snprintf(msg, sizeof msg, "%s: offset %d Hz at %d Hz has a mixer period above 2^20", who, (int) offsets_hz[k],
                     in_rate_hz);
            return fail(GNUAIS_E_ARG, msg);
        }
        off[k] = total;
        total += per[k];
    }
    std::vector<int16_t> mix(2 * (size_t) total);
    for (int k = 0; k < K; ++k) chan_mixer(in_rate_hz, offsets_hz[k], per[k], mix.data() + 2 * (size_t) off[k]);
    ResamplePlan p;
    if (na) resample_plan(up, down, h.data(), T, na, p);
    std::vector<int32_t> groups;
    if (na && rational)
        for (const ResampGroup &g : p.groups) groups.insert(groups.end(), {g.first, g.size, g.base});

    if (int rc = set_device(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->wide = WideStage{};
    WideStage w;
    HIP_TRY(w.mix.alloc(sizeof(uint32_t) * (size_t) total));
    HIP_TRY(hipMemcpy(w.mix, mix.data(), sizeof(uint32_t) * (size_t) total, hipMemcpyHostToDevice));
    if (int rc = to_device(w.taps, h)) return rc;
    if (int rc = to_device(w.poly, p.pairs)) return rc;
    if (int rc = to_device(w.groups, groups)) return rc;
    w.H = (T - 1 + up - 1) / up;
    if (w.H > 0)
        for (auto &q : w.hist) HIP_TRY(q.alloc(sizeof(uint32_t) * (size_t) w.H * (size_t) (b->N / K)));
    w.K = K;
    w.U = up;
    w.D = down;
    w.T = T;
    w.R = in_rate_hz;
    w.NA = na;
    for (int k = 0; k < K; ++k) { w.per[k] = per[k]; w.off[k] = off[k]; }
    b->wide = std::move(w);
    if (int rc = chan_zero_state(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return GNUAIS_OK;
}

int gnuais_batch_channeliser(gnuais_batch *b, int decim, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                             const int16_t *taps, int n_taps)
{
    if (!b || !offsets_hz) return fail(GNUAIS_E_ARG, "channeliser: NULL argument");
    if (decim < 1 || decim > 64) return fail(GNUAIS_E_ARG, "channeliser: decim must be 1..64");
    if (int rc = chan_shape_check(b, "channeliser", in_rate_hz, n_offsets)) return rc;
    std::vector<int16_t> h;
    if (!taps || n_taps == 0) resample_default_taps(1, decim, h);
    else if (n_taps < 1 || n_taps > 1025) return fail(GNUAIS_E_ARG, "channeliser: n_taps must be 1..1025");
    else h.assign(taps, taps + n_taps);
    // U = 1: the one phase is the whole prototype
    static const char *const why[] = {"", "", "channeliser: a tap is -32768 (|h| <= 32767)", "channeliser: sum |h| exceeds 65535"};
    if (const int r = resample_check_taps(1, h.data(), (int) h.size())) return fail(GNUAIS_E_ARG, why[r]);
    return wide_configure(b, "channeliser", 1, decim, in_rate_hz, offsets_hz, n_offsets, h,
                          channeliser_fast_na(n_offsets, (int) h.size(), decim), false);
}

// ---- wideband in at a rational ratio U/D (include/gnuais_hip.h) ----

static int resampler_ratio_check(const char *who, int up, int down)
{
    static const char *const why[] = {"", "up must be 1..64", "down must be 2..1024", "up must be below down (no up-sampling)",
                                      "up and down must have no common factor"};
    const int r = resample_check_ratio(up, down);
    if (!r) return GNUAIS_OK;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, why[r]);
    return fail(GNUAIS_E_ARG, msg);
}

static int resampler_taps_check(const char *who, int up, const int16_t *h, int T)
{
    static const char *const why[] = {"", "n_taps must be 1..16385", "a tap is -32768 (|h| <= 32767)",
                                      "a phase's sum |h[j]|, j = phase mod up, exceeds 65535"};
    const int r = resample_check_taps(up, h, T);
    if (!r) return GNUAIS_OK;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, why[r]);
    return fail(GNUAIS_E_ARG, msg);
}

int gnuais_resampler_default_taps(int up, int down, int16_t *out, int cap, int *n_taps)
{
    if (int rc = resampler_ratio_check("resampler_default_taps", up, down)) return rc;
    std::vector<int16_t> h;
    resample_default_taps(up, down, h);
    const int T = (int) h.size();
    if (n_taps) *n_taps = T;
    if (!out) return GNUAIS_OK;
    if (cap < T) return fail(GNUAIS_E_ARG, "resampler_default_taps: cap < 16*down + 1");
    memcpy(out, h.data(), sizeof(int16_t) * (size_t) T);
    return GNUAIS_OK;
}

int gnuais_resampler_plan(int up, int down, const int16_t *taps, int n_taps, int32_t *groups, int groups_cap,
                          uint32_t *pairs, int pairs_cap, int *n_pairs, int *n_acc, int *carry)
{
    if (int rc = resampler_ratio_check("resampler_plan", up, down)) return rc;
    std::vector<int16_t> h;
    if (!taps || n_taps == 0) resample_default_taps(up, down, h);
    else if (n_taps < 1 || n_taps > RESAMP_MAX_TAPS) return fail(GNUAIS_E_ARG, "resampler_plan: n_taps must be 1..16385");
    else h.assign(taps, taps + n_taps);
    if (int rc = resampler_taps_check("resampler_plan", up, h.data(), (int) h.size())) return rc;
    ResamplePlan p;
    // the stride the device's fast form reads (its one bucket); a longer prototype, the direct form's, at its own
    const int na = std::max(((int) h.size() + down - 1) / down, RESAMP_FAST_NA);
    resample_plan(up, down, h.data(), (int) h.size(), na, p);
    if (n_pairs) *n_pairs = p.n_pairs;
    if (n_acc) *n_acc = p.NA;
    if (carry) *carry = p.H;
    if (groups) {
        if (groups_cap < 3 * up) return fail(GNUAIS_E_ARG, "resampler_plan: groups_cap < 3 * up");
        memcpy(groups, p.groups.data(), sizeof(int32_t) * 3 * (size_t) up);
    }
    if (pairs) {
        if ((long long) pairs_cap < (long long) p.pairs.size()) return fail(GNUAIS_E_ARG, "resampler_plan: pairs_cap < n_pairs * n_acc");
        memcpy(pairs, p.pairs.data(), sizeof(uint32_t) * p.pairs.size());
    }
    return GNUAIS_OK;
}

int gnuais_batch_resampler(gnuais_batch *b, int up, int down, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                           const int16_t *taps, int n_taps)
{
    if (!b || !offsets_hz) return fail(GNUAIS_E_ARG, "resampler: NULL argument");
    if (int rc = resampler_ratio_check("resampler", up, down)) return rc;
    // the integer channeliser's own configuration and kernels: one path for U = 1, D <= 64
    if (up == 1 && down <= 64) return gnuais_batch_channeliser(b, down, in_rate_hz, offsets_hz, n_offsets, taps, n_taps);
    if (int rc = chan_shape_check(b, "resampler", in_rate_hz, n_offsets)) return rc;
    std::vector<int16_t> h;
    if (!taps || n_taps == 0) resample_default_taps(up, down, h);
    else if (n_taps < 1 || n_taps > RESAMP_MAX_TAPS) return fail(GNUAIS_E_ARG, "resampler: n_taps must be 1..16385");
    else h.assign(taps, taps + n_taps);
    if (int rc = resampler_taps_check("resampler", up, h.data(), (int) h.size())) return rc;
    return wide_configure(b, "resampler", up, down, in_rate_hz, offsets_hz, n_offsets, h,
                          resampler_fast_na(n_offsets, (int) h.size(), down), true);
}

// The checks of the entries that take a form's input, in the name of the entry `who` (the device entries of the
// narrowband forms add "(max_len)" to the len message, as gnuais_batch_run does); fmt: the wide form's sample format
static int check_input(const gnuais_batch *b, FormId id, const void *x, int len, const char *who, bool host,
                       int fmt = GNUAIS_FMT_CS16)
{
    char msg[200];
    if (!b || !x) {
        snprintf(msg, sizeof msg, "%s: NULL argument", who);
    } else if (id != WIDE) {
        if (len > 0 && len <= b->max_len) return GNUAIS_OK;
        snprintf(msg, sizeof msg, "%s: len out of range%s", who, host ? "" : " (max_len)");
    } else if (!wide_format_bytes(fmt)) {
        snprintf(msg, sizeof msg, "%s: unknown sample format %d (GNUAIS_FMT_*)", who, fmt);
    } else if (!b->wide.K) {
        snprintf(msg, sizeof msg, "%s: no channeliser configured (call gnuais_batch_channeliser first)", who);
    } else if (b->wide.U == 1 && (len <= 0 || len % b->wide.D || len / b->wide.D > b->max_len)) {
        snprintf(msg, sizeof msg, "%s: len %d must be a positive multiple of the decimation %d, at most %d * max_len", who,
                 len, b->wide.D, b->wide.D);
    } else if (len <= 0 || len % b->wide.D || (long long) (len / b->wide.D) * b->wide.U > b->max_len) {
        snprintf(msg, sizeof msg, "%s: len %d must be a positive multiple of down = %d that gives at most max_len rows "
                 "(len * %d / %d <= %d)", who, len, b->wide.D, b->wide.U, b->wide.D, b->max_len);
    } else if (reinterpret_cast<uintptr_t>(x) % (uintptr_t) wide_format_align(fmt)) {
        snprintf(msg, sizeof msg, "%s: %s wide samples must be %d-byte aligned", who, wide_format_name(fmt),
                 wide_format_align(fmt));
    } else {
        return GNUAIS_OK;
    }
    return fail(GNUAIS_E_ARG, msg);
}

static int chan_launch(gnuais_batch *b, int fmt, const void *d_wide, int len, int16_t *d_out, hipStream_t s)
{
    WideStage &w = b->wide;
    WideLaunch a{};
    a.in = d_wide;
    a.out = reinterpret_cast<uint32_t *>(d_out);
    a.hist = w.hist[w.cur];
    a.mix = w.mix;
    a.poly = w.poly;
    a.groups = w.groups;
    a.taps = w.taps;
    a.M = b->N / w.K;
    a.K = w.K;
    a.U = w.U;
    a.D = w.D;
    a.T = w.T;
    a.H = w.H;
    a.len = len;
    // the fast form stores K words per lane as one vector: the output must be aligned to it (else the direct form)
    const unsigned vec = a.K == 2 ? 8u : a.K == 4 ? 16u : 4u;
    a.NA = (reinterpret_cast<uintptr_t>(d_out) % vec) ? 0 : w.NA;
    if (reinterpret_cast<uintptr_t>(d_out) % 4) return fail(GNUAIS_E_ARG, "channelise: the output must be 4-byte aligned");
    for (int k = 0; k < a.K; ++k) {
        a.per[k] = w.per[k];
        a.off[k] = w.off[k];
        a.ph0[k] = (int) (w.n % (unsigned long long) w.per[k]);
    }
    HIP_TRY(launch_wide(a, fmt, w.hist[w.cur ^ 1], s));
    if (w.H > 0) w.cur ^= 1;
    w.n += (unsigned long long) len;
    b->last[CHAN] = {s, true};
    return GNUAIS_OK;
}

static int channelise(gnuais_batch *b, int fmt, const void *d_wide, int len, int16_t *d_out, void *stream, const char *who)
{
    if (int rc = check_input(b, WIDE, d_wide, len, who, false, fmt)) return rc;
    if (!d_out) return fail(GNUAIS_E_ARG, (std::string(who) + ": NULL argument").c_str());
    if (int rc = set_device(b)) return rc;
    if (int rc = drain(b, 1u << CHAN, (hipStream_t) stream)) return rc;
    return chan_launch(b, fmt, d_wide, len, d_out, (hipStream_t) stream);
}

int gnuais_batch_channelise(gnuais_batch *b, const int16_t *d_wide, int len, int16_t *d_out, void *stream)
{
    return channelise(b, GNUAIS_FMT_CS16, d_wide, len, d_out, stream, "channelise");
}

int gnuais_batch_channelise_fmt(gnuais_batch *b, int fmt, const void *d_wide, int len, int16_t *d_out, void *stream)
{
    return channelise(b, fmt, d_wide, len, d_out, stream, "channelise_fmt");
}

// ---- the signal power and carrier error of every frame (include/gnuais_hip.h, frame_signal.hip) ----

// In front of the discriminator of an I/Q-type call, on its stream s (the discriminator's entry of the drain table covers
// it: same calls, same stream): the block sums of the call's rows.  The chain has taken b->rows rows: the call's first is n0.
static int power_launch(gnuais_batch *b, const int16_t *d_iq, int len, hipStream_t s)
{
    if (b->rows != b->fs_end) b->fs_v0 = b->rows;        // an audio-type call came between: a new run starts here
    HIP_TRY(launch_iq_power(d_iq, b->fs_carry, b->fs_ring, b->fs_RB, b->N, len, b->rows, b->rows == b->fs_v0, s));
    b->fs_end = b->rows + (unsigned long long) len;      // a run call that fails leaves rows behind it: a new run next time
    if (b->occ_E) {
        // gnuais_batch_occupancy: a new run drops the epochs of the last one that are not final and counts from its own
        // first whole block; then the codes of the blocks this call completed, on the same stream behind their sums
        if (b->rows == b->fs_v0) {
            b->occ_v0 = b->rows;
            b->occ_next = 0;
        }
        const long long j0 = std::max(occ_b0(b), (long long) (b->rows / FS_BLOCK)), j1 = (long long) (b->fs_end / FS_BLOCK);
        if (j1 > j0) HIP_TRY(launch_occ_code(b->fs_ring, b->fs_RB, b->occ_codes, b->occ_CB, b->N, j0, (int) (j1 - j0), s));
    }
    return GNUAIS_OK;
}

static int fs_ring_alloc(gnuais_batch *b, bool long_span, const char *who);

// Synchronises: no call is in flight when the switch turns.  The records of what the ring holds start at (0, 0, 0), the
// run of I/Q-type calls at the current row.
int gnuais_batch_frame_signal(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "frame_signal: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "frame_signal: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (on && !b->frame_times)
        return fail(GNUAIS_E_STATE, "frame_signal: the batch does not time its frames (gnuais_batch_frame_times): a frame's "
                                    "span is found by its receive time");
    if (!on && b->occ_E)
        return fail(GNUAIS_E_STATE, "frame_signal: the batch codes the block sums of this ring (gnuais_batch_occupancy); "
                                    "gnuais_batch_occupancy(b, 0, 0) first");
    if (!on && b->long_frame_signal)
        return fail(GNUAIS_E_STATE, "frame_signal: the batch measures its long frames from this ring "
                                    "(gnuais_batch_long_frame_signal); gnuais_batch_long_frame_signal(b, 0) first");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->frame_signal = false;
    HIP_TRY(b->fs_ring.release());
    b->fs_long = false;
    if (!on) return GNUAIS_OK;
    if (int rc = fs_ring_alloc(b, b->long_frame_signal, "frame_signal")) return rc;
    const size_t N = (size_t) b->N;
    HIP_TRY(b->fs_carry.ensure(sizeof(uint32_t) * N));
    HIP_TRY(b->signal.ensure(sizeof(gnuais_frame_signal) * (size_t) b->frame_cap));
    HIP_TRY(hipMemset(b->signal, 0, sizeof(gnuais_frame_signal) * (size_t) b->frame_cap));
    b->frame_signal = true;
    return GNUAIS_OK;
}

// The ring of block sums anew (the device is idle), sized for frames of 448 bits, or of GNUAIS_LONG_MAX_BITS with
// long_span; the run of I/Q-type calls starts at the current row.  A failure leaves the batch without a ring.
static int fs_ring_alloc(gnuais_batch *b, bool long_span, const char *who)
{
    HIP_TRY(b->fs_ring.release());
    // The ring's size.  No slot may be written while a frame launch that can still read it is pending.  The ingest
    // launch of call i is queued before the host waits for the tail of call i - nbuf (gnuais_batch_run: e_done[4][k]),
    // so while the frame launch of call c is pending, ingest launches up to call c + nbuf may run: they write rows
    // below n0_c + (nbuf + 1) * max_len.  That frame launch reads from row q - S on, q = t - d_f - W/2 with t >= n0_c:
    // at most S_max + d_f + W_max/2 rows below n0_c, S_max the span of the longest frame (448 bits; 1008 with long_span:
    // the launch of long_signal.hip is queued where the frame launch is, in the same tail, and reads a longer span from
    // the same q on, so the argument holds with the longer S_max).  nbuf + 2 calls
    // instead of nbuf + 1 leave one call of slack; one block more at either end for the two open ones.
    // That wait belongs to the pipelined path.  With the pipeline off (set_option("pipeline", 0)) a call's tail runs on
    // the caller's stream behind its K1, so on one stream the next call's ingest launch is behind the pending frame
    // launch in stream order, and a call on another stream drains the chain's recorded stream first (run_form passes
    // the CHAIN bit to drain()): no ingest launch ever runs beside a pending frame launch there.
    const long long S_max = fs_span_rows(long_span ? FS_LONG_MAX_NBITS : FS_MAX_NBITS, b->pllinc);
    const long long rows = (long long) (b->nbuf + 2) * b->max_len + S_max + (b->NT + 1) / 2 + AFC_MAX_WINDOW / 2;
    const long long RB = fs_ceil_div(rows, FS_BLOCK) + 2;
    if (S_max / FS_BLOCK + 1 > 0xffff || RB > 0x7fffffff) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: the batch's pllinc gives frames of more than 65535 blocks", who);
        return fail(GNUAIS_E_STATE, msg);
    }
    const size_t N = (size_t) b->N;
    if (int rc = alloc_checked(b, b->fs_ring, sizeof(int64_t) * 3 * N * (size_t) RB, who, "the ring of block sums"))
        return rc;
    b->fs_RB = (int) RB;
    b->fs_nbuf = b->nbuf;
    b->fs_v0 = b->fs_end = b->rows;
    b->fs_long = long_span;
    return GNUAIS_OK;
}

// ---- the signal record of every long frame (include/gnuais_hip.h, long_signal.hip) ----

// Synchronises: no call is in flight when the switch turns, so every D' launch either has the long signal launch behind
// it or has not.  Switching on re-sizes the ring of block sums for the 1008-bit span and starts a new run of I/Q-type
// calls at the current row, as switching gnuais_batch_frame_signal on does; the records of the short frames already
// queued stay as they are, those of the long frames already queued are (0, 0, 0).  Switching off keeps the ring.
int gnuais_batch_long_frame_signal(gnuais_batch *b, int on)
{
    if (!b) return fail(GNUAIS_E_ARG, "long_frame_signal: NULL batch");
    if (!b->long_frames)
        return fail(GNUAIS_E_STATE, "long_frame_signal: the batch does not decode long frames (gnuais_batch_long_frames): "
                                    "the records measured are that decoder's");
    if (!b->frame_signal)
        return fail(GNUAIS_E_STATE, "long_frame_signal: the batch keeps no block sums (gnuais_batch_frame_signal): a long "
                                    "frame's record is the sum of its blocks");
    if (b->occ_E)
        return fail(GNUAIS_E_STATE, "long_frame_signal: the rings of gnuais_batch_occupancy are sized for the frames that "
                                    "covered when it was switched on; gnuais_batch_occupancy(b, 0, 0) first");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->long_frame_signal = false;
    if (!on) return GNUAIS_OK;
    if (int rc = fs_ring_alloc(b, true, "long_frame_signal")) {
        b->frame_signal = false;                // the ring is gone: gnuais_batch_frame_signal(b, 1) makes a new one
        return rc;
    }
    HIP_TRY(b->long_signal.ensure(sizeof(gnuais_frame_signal) * (size_t) b->long_cap));
    HIP_TRY(hipMemset(b->long_signal, 0, sizeof(gnuais_frame_signal) * (size_t) b->long_cap));
    b->long_frame_signal = true;
    return GNUAIS_OK;
}

// a parity tap: the ring's sums of the blocks [j0, j0 + count), h_out [count][N][3] (P, R, I)
int gnuais_batch_signal_blocks(gnuais_batch *b, long long j0, int count, int64_t *h_out)
{
    if (!b || count < 0 || (count > 0 && !h_out)) return fail(GNUAIS_E_ARG, "signal_blocks: argument");
    if (!b->frame_signal) return fail(GNUAIS_E_STATE, "signal_blocks: the batch does not measure its frames (gnuais_batch_frame_signal)");
    if (int rc = set_device(b)) return rc;
    // what the ring holds: the blocks of the current run, the one v0 lies in included, that later ones have not replaced
    const long long end = (long long) ((b->fs_end + FS_BLOCK - 1) / FS_BLOCK);
    const long long lo = std::max((long long) (b->fs_v0 / FS_BLOCK), end - b->fs_RB);
    if (j0 < lo || j0 + count > end) {
        char msg[200];
        snprintf(msg, sizeof msg, "signal_blocks: blocks [%lld, %lld) asked for, the ring holds [%lld, %lld)", j0, j0 + count, lo, end);
        return fail(GNUAIS_E_ARG, msg);
    }
    if (b->last[DISC].used) HIP_TRY(hipStreamSynchronize(b->last[DISC].s));
    const size_t blk = 3 * (size_t) b->N;
    for (int k = 0; k < count; ++k)
        HIP_TRY(hipMemcpy(h_out + (size_t) k * blk, b->fs_ring + (size_t) ((j0 + k) % b->fs_RB) * blk, sizeof(int64_t) * blk,
                          hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

// ---- the channel load per receiver (include/gnuais_hip.h, occupancy.hip) ----

// Synchronises: no call is in flight when the switch turns.  The run the epochs are counted in starts at the current row.
int gnuais_batch_occupancy(gnuais_batch *b, int epoch_blocks, int margin)
{
    if (!b) return fail(GNUAIS_E_ARG, "occupancy: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "occupancy: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    if (epoch_blocks && !b->frame_signal)
        return fail(GNUAIS_E_STATE, "occupancy: the batch keeps no block sums (gnuais_batch_frame_signal): a block's code is "
                                    "the code of its sum");
    if (epoch_blocks && (epoch_blocks < OCC_MIN_EPOCH || epoch_blocks > OCC_MAX_EPOCH || margin < 1 || margin > 255))
        return fail(GNUAIS_E_ARG, "occupancy: epoch_blocks must be 0 (off) or 64..4096, margin 1..255");
    if (int rc = gnuais_batch_sync(b)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->occ_E = 0;
    b->occ_long = false;
    HIP_TRY(b->occ_codes.release());
    HIP_TRY(b->occ_cover.release());
    if (!epoch_blocks) return GNUAIS_OK;
    // The rings' size.  No slot may be written while a finaliser that can still read it is pending.  The finaliser of
    // the epoch of the blocks [f, f + E) is queued in the tail of the first call c whose rows end behind row
    // 64 (f + E) - 1 + LAG, so that call begins at or before that row: n0_c <= 64 (f + E) - 1 + LAG.  As for the signal
    // ring (gnuais_batch_frame_signal above), while the tail of call c is pending the ingest side of up to call c + nbuf
    // may run, and its code launches write blocks whose rows lie below n0_c + (nbuf + 1) * max_len; the cover launch of
    // call c itself stores up to row n0_c + len + S_post.  All of them are blocks below
    // f + E + ceil(LAG / 64) + (nbuf + 1) * ceil(max_len / 64) + 1, and the finaliser reads and writes from block f on.
    // nbuf + 2 calls instead of nbuf + 1 leave one call of slack, one block more for the open one.  LAG is that of the
    // AFC window in use; gnuais_batch_afc refuses a wider one while the feature is on.  With the pipeline off every
    // launch is in one stream's order, as there.  Where the long frames cover too (gnuais_batch_long_frame_signal is on
    // at this switch), LAG is that of the 1008-bit span and their cover launch sits where the chain's does, in the same
    // tail in front of the same finalisers, and stores up to the same row: the argument holds with the longer LAG.
    b->occ_long = b->long_frame_signal;
    const long long lag = occ_lag_rows(b->pllinc, b->NT, b->afc_W, occ_max_nbits(b));
    const long long CB = epoch_blocks + fs_ceil_div(lag, FS_BLOCK) + (long long) (b->nbuf + 2) * fs_ceil_div(b->max_len, FS_BLOCK) + 2;
    if (CB > 0x7fffffff) return fail(GNUAIS_E_STATE, "occupancy: the batch's pllinc gives frames of more than 2^31 blocks");
    const size_t N = (size_t) b->N;
    if (int rc = alloc_checked(b, b->occ_codes, sizeof(uint16_t) * N * (size_t) CB, "occupancy", "the ring of block codes"))
        return rc;
    if (int rc = alloc_checked(b, b->occ_cover, N * (size_t) CB, "occupancy", "the ring of cover bytes")) return rc;
    HIP_TRY(hipMemset(b->occ_cover, 0, N * (size_t) CB));
    HIP_TRY(b->occ_carry.ensure(N));
    HIP_TRY(hipMemset(b->occ_carry, 0, N));
    HIP_TRY(b->occ_out.ensure(sizeof(gnuais_occupancy) * N * OCC_RING_EPOCHS));
    b->occ_CB = (int) CB;
    b->occ_nbuf = b->nbuf;
    b->occ_W = b->afc_W;
    b->occ_margin = margin;
    b->occ_cover_clean = true;
    b->occ_E = epoch_blocks;
    return occ_zero_state(b);
}

// the final epochs in order: h_out [max][N], h_first_block [max]
int gnuais_batch_drain_occupancy(gnuais_batch *b, gnuais_occupancy *h_out, int64_t *h_first_block, int max, int *n_out)
{
    if (!b || !n_out || max < 0 || (max > 0 && (!h_out || !h_first_block))) return fail(GNUAIS_E_ARG, "drain_occupancy: argument");
    *n_out = 0;
    if (!b->occ_E) return fail(GNUAIS_E_STATE, "drain_occupancy: the batch does not measure its channels' load (gnuais_batch_occupancy)");
    if (int rc = set_device(b)) return rc;
    if (b->occ_drained == b->occ_seq || max == 0) return GNUAIS_OK;
    if (int rc = gnuais_batch_sync(b)) return rc;              // the tails that produced them
    const size_t N = (size_t) b->N;
    int n = 0;
    for (; n < max && b->occ_drained < b->occ_seq; ++n, ++b->occ_drained) {
        const int slot = (int) (b->occ_drained % OCC_RING_EPOCHS);
        HIP_TRY(hipMemcpy(h_out + (size_t) n * N, b->occ_out.p + (size_t) slot * N, sizeof(gnuais_occupancy) * N, hipMemcpyDeviceToHost));
        h_first_block[n] = b->occ_first[slot];
    }
    *n_out = n;
    return GNUAIS_OK;
}

int gnuais_batch_occupancy_lost(gnuais_batch *b, long long *lost)
{
    if (!b || !lost) return fail(GNUAIS_E_ARG, "occupancy_lost: argument");
    *lost = b->occ_lost;
    return GNUAIS_OK;
}

// the tap: the words code | busy << 14 | cover << 15 of the blocks [j0, j0 + count), h_out [count][N]
int gnuais_batch_occupancy_blocks(gnuais_batch *b, long long j0, int count, uint16_t *h_out)
{
    if (!b || count < 0 || (count > 0 && !h_out)) return fail(GNUAIS_E_ARG, "occupancy_blocks: argument");
    if (!b->occ_E) return fail(GNUAIS_E_STATE, "occupancy_blocks: the batch does not measure its channels' load (gnuais_batch_occupancy)");
    if (int rc = set_device(b)) return rc;
    // what the ring holds of final epochs: those of the current run that the codes of later blocks have not replaced
    const long long end = occ_b0(b) + b->occ_next * b->occ_E;
    const long long lo = std::max(occ_b0(b), (long long) (b->fs_end / FS_BLOCK) - b->occ_CB);
    if (j0 < lo || j0 + count > end) {
        char msg[200];
        snprintf(msg, sizeof msg, "occupancy_blocks: blocks [%lld, %lld) asked for, the ring holds the final blocks [%lld, %lld)",
                 j0, j0 + count, lo, std::max(lo, end));
        return fail(GNUAIS_E_ARG, msg);
    }
    if (int rc = gnuais_batch_sync(b)) return rc;
    const size_t N = (size_t) b->N;
    for (int k = 0; k < count; ++k)
        HIP_TRY(hipMemcpy(h_out + (size_t) k * N, b->occ_codes + (size_t) ((j0 + k) % b->occ_CB) * N, sizeof(uint16_t) * N,
                          hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

// ---- one run path and one host path for every input form ----

// gnuais_batch_run_iq / _run_wideband: on the caller's stream, the stages in front of the chain, each into the
// intermediate buffer that the next one reads, then gnuais_batch_run on the audio.  in: the form's input, wide samples in
// format fmt
static int run_form(gnuais_batch *b, FormId id, const void *in, int len, void *stream, const char *who,
                    int fmt = GNUAIS_FMT_CS16)
{
    if (int rc = check_input(b, id, in, len, who, false, fmt)) return rc;
    if (int rc = set_device(b)) return rc;
    const Form f = form(b, id);
    const bool chan = f.stages >> CHAN & 1u, disc = f.stages >> DISC & 1u, afc = f.stages >> AFC & 1u;
    hipStream_t s = (hipStream_t) stream;
    if (int rc = drain(b, f.stages, s)) return rc;
    // the channeliser writes max_len rows of the I/Q form, the discriminator and the AFC max_len rows of the audio form
    if (chan)
        if (int rc = alloc_checked(b, b->wide_iq, form(b, IQ).bytes_of(b->max_len), who, "the channeliser's I/Q")) return rc;
    if (disc)
        if (int rc = alloc_checked(b, b->iq_audio, form(b, AUDIO).bytes_of(b->max_len), who, "the discriminator's audio"))
            return rc;
    if (afc)
        if (int rc = alloc_checked(b, b->afc_audio, form(b, AUDIO).bytes_of(b->max_len), who, "the AFC's audio")) return rc;
    const int16_t *x = static_cast<const int16_t *>(in);
    if (chan) {
        if (int rc = chan_launch(b, fmt, in, len, b->wide_iq, s)) return rc;
        x = b->wide_iq;
    }
    len = len / f.rows * f.up;
    if (b->frame_signal)
        if (int rc = power_launch(b, x, len, s)) return rc;
    if (disc) {
        if (int rc = disc_launch(b, x, len, b->iq_audio, s, afc)) return rc;
        x = b->iq_audio;
    }
    if (afc) {
        if (int rc = afc_launch(b, x, len, b->afc_audio, s)) return rc;
        x = b->afc_audio;
    }
    b->fs_iq_call = b->frame_signal;            // the chain's rows of this call are I/Q rows (fill_frame_signal)
    const int rc = gnuais_batch_run(b, x, len, stream);
    b->fs_iq_call = false;
    return rc;
}

// gnuais_batch_run_host / _run_iq_host / _run_wideband_host: the host input staged in stage_x, then `run`, the
// device entry of the same form, on the NULL stream, then a sync.  run == NULL: the wide form in format fmt, through
// gnuais_batch_run_wideband_fmt; its bytes are those of the format: nothing is widened on the host
static int run_staged(gnuais_batch *b, FormId id, const void *h, int len, const char *who,
                      int (*run)(gnuais_batch *, const int16_t *, int, void *), int fmt = GNUAIS_FMT_CS16)
{
    if (int rc = check_input(b, id, h, len, who, true, fmt)) return rc;
    if (int rc = set_device(b)) return rc;
    const size_t bytes = form(b, id, fmt).bytes_of(len);
    HIP_TRY(b->stage_x.grow(bytes));
    HIP_TRY(hipMemcpy(b->stage_x, h, bytes, hipMemcpyHostToDevice));
    if (int rc = run ? run(b, b->stage_x, len, nullptr) : gnuais_batch_run_wideband_fmt(b, fmt, b->stage_x, len, nullptr))
        return rc;
    return gnuais_batch_sync(b);
}

int gnuais_batch_run_iq(gnuais_batch *b, const int16_t *d_iq, int len, void *stream)
{
    return run_form(b, IQ, d_iq, len, stream, "run_iq");
}

int gnuais_batch_run_wideband(gnuais_batch *b, const int16_t *d_wide, int len, void *stream)
{
    return run_form(b, WIDE, d_wide, len, stream, "run_wideband");
}

int gnuais_batch_run_host(gnuais_batch *b, const int16_t *h_samples, int len)
{
    return run_staged(b, AUDIO, h_samples, len, "run_host", gnuais_batch_run);
}

int gnuais_batch_run_iq_host(gnuais_batch *b, const int16_t *h_iq, int len)
{
    return run_staged(b, IQ, h_iq, len, "run_iq_host", gnuais_batch_run_iq);
}

int gnuais_batch_run_wideband_host(gnuais_batch *b, const int16_t *h_wide, int len)
{
    return run_staged(b, WIDE, h_wide, len, "run_wideband_host", gnuais_batch_run_wideband);
}

int gnuais_batch_run_wideband_fmt(gnuais_batch *b, int fmt, const void *d_wide, int len, void *stream)
{
    return run_form(b, WIDE, d_wide, len, stream, "run_wideband_fmt", fmt);
}

int gnuais_batch_run_wideband_fmt_host(gnuais_batch *b, int fmt, const void *h_wide, int len)
{
    return run_staged(b, WIDE, h_wide, len, "run_wideband_fmt_host", nullptr, fmt);
}

int gnuais_batch_run_host_async(gnuais_batch *b, const int16_t *h_samples, int len)
{
    if (!b || !h_samples) return fail(GNUAIS_E_ARG, "run_host_async: NULL argument");
    if (len <= 0 || len > b->max_len) return fail(GNUAIS_E_ARG, "run_host_async: len out of range");
    if (int rc = set_device(b)) return rc;
    const size_t bytes = sizeof(int16_t) * (size_t) len * (size_t) b->N;
    HIP_TRY(b->s_io.ensure());
    for (auto &e : b->e_in) HIP_TRY(e.ensure(hipEventDisableTiming));
    if (b->pin_bytes < bytes) {                 // (re)size for the largest call seen
        HIP_TRY(hipStreamSynchronize(b->s_io));
        const size_t cap = sizeof(int16_t) * (size_t) b->max_len * (size_t) b->N;
        const size_t want = std::min(cap, std::max(bytes, (size_t) 1 << 20));
        for (int q = 0; q < 2; ++q) {              // all four go before any comes back
            HIP_TRY(b->pin[q].release());
            HIP_TRY(b->dev_in[q].release());
        }
        b->pin_bytes = 0;
        for (int q = 0; q < 2; ++q) {
            HIP_TRY(b->pin[q].alloc(want));
            HIP_TRY(b->dev_in[q].alloc(want));
        }
        b->pin_bytes = want;
        b->host_calls = 0;
    }
    const int q = (int) (b->host_calls & 1);
    // the pair was last used two calls ago: its transfer and the FIR that read it must be done
    if (b->host_calls >= 2) HIP_TRY(hipEventSynchronize(b->e_in[q]));
    memcpy(b->pin[q], h_samples, bytes);
    HIP_TRY(hipMemcpyAsync(b->dev_in[q], b->pin[q], bytes, hipMemcpyHostToDevice, b->s_io));
    b->e_in_hook = b->e_in[q];                  // recorded right behind K1 (run_chain): K1 is the input's only reader
    const int rc = gnuais_batch_run(b, b->dev_in[q], len, b->s_io);
    if (b->e_in_hook) {                         // the run failed before its K1: whatever s_io holds (the copy) guards the pair
        b->e_in_hook = nullptr;
        (void) hipEventRecord(b->e_in[q], b->s_io);
    }
    b->host_calls++;                            // also after a failed run: the copy from pin[q] may still be in flight
    return rc;
}

} // extern "C"
