// capi_delivery.hip -- the C ABI's output side (include/gnuais_hip.h): what becomes of the frames K3 has appended to the
// batch's ring -- the drains, the messages and vessel folds, the vessel table carried on the device, the streamed
// delivery (gnuais_batch_stream_nmea) and the placement of its copy stream.  Host code only.
#include "batch.h"

// A pending discard as the memset it used to be: behind the last K3 (not pipelined: on the stream the discard named).  Everything that
// reads or hands out ring 0 or its words without a deframer launch in between comes through here first.
int gnuais::discard_flush(gnuais_batch *b)
{
    if (!b->discard_pending) return GNUAIS_OK;
    b->discard_pending = false;
    hipStream_t s = b->pipeline ? k3_stream(b) : b->discard_stream;     // behind the last K3
    HIP_TRY(hipMemsetAsync(b->ring_count[0], 0, sizeof(uint32_t) * 3, s));
    return GNUAIS_OK;
}

extern "C" {

// device buffers of the post-stage (sorted records / text, rocPRIM scratch): allocated on first use
static int ensure_post_buffers(gnuais_batch *b, uint32_t have)
{
    const size_t need_text = (size_t) have * 164, need_scratch = nmea_scratch_bytes((int) have);
    HIP_TRY(b->d_text.grow(need_text));
    HIP_TRY(b->nmea_scratch.grow(need_scratch));
    return GNUAIS_OK;
}

// What is queued in the ring of a batch that does not stream, once the chain is idle: `have` frames; `overflow`: more
// came than the ring holds; `watchdog`: a PLL-stage wave timed out waiting for its partner
struct Pending {
    uint32_t have;
    bool overflow, watchdog;
};

static int read_pending(gnuais_batch *b, Pending &p)
{
    if (int rc = discard_flush(b)) return rc;
    if (int rc = gnuais_batch_sync(b)) return rc;
    uint32_t cnt[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(cnt, b->ring_count[0], sizeof cnt, hipMemcpyDeviceToHost));
    p.have = std::min<uint32_t>(cnt[0], (uint32_t) b->frame_cap);
    p.overflow = cnt[1] || cnt[0] > (uint32_t) b->frame_cap;
    p.watchdog = cnt[3] != 0;
    return GNUAIS_OK;
}

// the two errors a span of frames reports late, with what it delivered, in the name of the entry `who`
static int late_error(const char *who, bool watchdog, bool overflow, const char *watchdog_tail = "")
{
    char msg[200];
    if (watchdog) {
        snprintf(msg, sizeof msg, "%s: the PLL stage's watchdog fired (device hung or badly oversubscribed)%s", who, watchdog_tail);
        return fail(GNUAIS_E_HIP, msg);
    }
    if (!overflow) return GNUAIS_OK;
    snprintf(msg, sizeof msg, "%s: frame ring overflowed, frames were dropped", who);
    return fail(GNUAIS_E_OVERFLOW, msg);
}

// the end of a drain that consumes: the ring is empty again, then the late errors
static int finish_drain(gnuais_batch *b, const Pending &p, const char *who, const char *watchdog_tail = "")
{
    HIP_TRY(hipMemset(b->ring_count[0], 0, sizeof(uint32_t) * 4));
    b->hdlc_calls = 0;
    return late_error(who, p.watchdog, p.overflow, watchdog_tail);
}

// the caller's sequence digits into d_seq[0] and, for the formatter to advance, d_seq[1] (allocated on first use)
static int upload_seq(gnuais_batch *b, const uint8_t *seqnr)
{
    const size_t N = (size_t) b->N;
    for (auto &p : b->d_seq) HIP_TRY(p.ensure(N));
    HIP_TRY(hipMemcpy(b->d_seq[0], seqnr, N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_seq[1], b->d_seq[0], N, hipMemcpyDeviceToDevice));
    return GNUAIS_OK;
}

// drain: records and / or sentences of everything queued, consumed once
// h_times (with h_frames): the records' receive times, through the sort's own permutation; h_signal (with h_times):
// their power and carrier error, likewise
static int drain_impl(gnuais_batch *b, gnuais_frame *h_frames, int max_frames, int *n_frames,
                      uint8_t *seqnr, char *out, size_t out_cap, size_t *out_len, int *n_sentences,
                      int64_t *h_times = nullptr, gnuais_frame_signal *h_signal = nullptr)
{
    // a streaming batch spreads its frames over NRING rings that gnuais_batch_stream_nmea() consumes: ring 0 alone
    // would be a partial view, and clearing its counters would lose frames and error flags
    if (b->streaming) return fail(GNUAIS_E_STATE, "drain: the batch is streaming (gnuais_batch_stream_nmea); "
                                                  "set_option(\"streaming\", 0) leaves that mode");
    Pending pend;
    if (int rc = read_pending(b, pend)) return rc;
    const uint32_t have = pend.have;
    if (h_frames && (uint32_t) max_frames < have) return fail(GNUAIS_E_ARG, "drain: frame buffer too small");
    if (have) {
        const size_t N = (size_t) b->N;
        if (int rc = ensure_post_buffers(b, have)) return rc;
        if (seqnr) {
            // sentences first (the formatter sorts for itself and leaves the ring untouched)
            if (int rc = upload_seq(b, seqnr)) return rc;
            uint32_t info[3] = {0, 0, 0};
            HIP_TRY(nmea_format(b->ring[0], (int) have, b->N, b->d_seq[0], b->d_seq[1], b->d_text, b->d_text.bytes,
                                b->nmea_scratch, b->nmea_scratch.bytes, info, nullptr));
            if (info[2]) return fail(GNUAIS_E_HIP, "drain: a frame record names a channel outside the batch");
            if ((size_t) info[0] > out_cap) {
                *out_len = info[0];
                return fail(GNUAIS_E_ARG, "drain: text buffer too small");
            }
            if (info[0]) HIP_TRY(hipMemcpy(out, b->d_text, info[0], hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(seqnr, b->d_seq[1], N, hipMemcpyDeviceToHost));
            *out_len = info[0];
            if (n_sentences) *n_sentences = (int) info[1];
        }
        if (h_frames) {
            // K3 appends the frames in pieces, in whatever order its blocks finish; the reference's
            // print order (channel, then time) is restored on the device -- radix sort of
            // (channel, end_bit), gather -- and the records cross PCIe once, straight into h_frames
            // (the text buffer holds 164 bytes per frame: the 64 of a record, the 8 of its time and the 8 of its signal
            // record fit side by side)
            static_assert(sizeof(gnuais_frame_signal) == sizeof(int64_t), "the signal records leave through the times' gather");
            gnuais_frame *sorted = reinterpret_cast<gnuais_frame *>(b->d_text.p);
            int64_t *sorted_t = reinterpret_cast<int64_t *>(sorted + have), *sorted_s = sorted_t + have;
            HIP_TRY(frames_sort_timed(b->ring[0], h_times ? b->times.p : nullptr, (int) have, sorted, sorted_t,
                                      b->nmea_scratch, b->nmea_scratch.bytes, nullptr,
                                      h_signal ? reinterpret_cast<const int64_t *>(b->signal.p) : nullptr, sorted_s));
            HIP_TRY(hipMemcpy(h_frames, sorted, sizeof(gnuais_frame) * have, hipMemcpyDeviceToHost));
            if (h_times) HIP_TRY(hipMemcpy(h_times, sorted_t, sizeof(int64_t) * have, hipMemcpyDeviceToHost));
            if (h_signal) HIP_TRY(hipMemcpy(h_signal, sorted_s, sizeof(gnuais_frame_signal) * have, hipMemcpyDeviceToHost));
        }
        if (n_frames) *n_frames = (int) have;
    }
    return finish_drain(b, pend, "drain", "; results are incomplete");
}

// Row f1 complete on the device: sentences AND stdout lines of everything queued, consumed once
int gnuais_batch_drain_messages(gnuais_batch *b, uint8_t *seqnr, const char *chanid, char *nmea, size_t nmea_cap,
                                size_t *nmea_len, int *n_sentences, char *text, size_t text_cap, size_t *text_len,
                                int *n_lines, int *n_frames)
{
    if (!b || !seqnr || !nmea_len || !text_len || (nmea_cap && !nmea) || (text_cap && !text))
        return fail(GNUAIS_E_ARG, "drain_messages: argument");
    if (b->streaming) return fail(GNUAIS_E_ARG, "drain_messages: the batch is streaming (gnuais_batch_stream_nmea)");
    *nmea_len = *text_len = 0;
    if (n_sentences) *n_sentences = 0;
    if (n_lines) *n_lines = 0;
    if (n_frames) *n_frames = 0;
    Pending pend;
    if (int rc = read_pending(b, pend)) return rc;
    const uint32_t have = pend.have;
    if (have) {
        const size_t N = (size_t) b->N, line = messages_line_bytes();
        if (nmea_cap < (size_t) have * 164 || text_cap < (size_t) have * line)
            return fail(GNUAIS_E_ARG, "drain_messages: buffers too small (164 / 512 bytes per pending frame always suffice)");
        if (int rc = ensure_post_buffers(b, have)) return rc;
        // lines at a fixed stride, their lengths and offsets, the packed text, two info words, the channel names
        const size_t need = (size_t) have * line * 2 + (size_t) have * 8 + 256 + N + 256;
        HIP_TRY(b->d_msg.grow(need, need / 4));
        char *lines = b->d_msg, *packed = lines + (size_t) have * line;
        uint32_t *len = reinterpret_cast<uint32_t *>(packed + (size_t) have * line), *off = len + have;
        uint32_t *info2 = off + have;
        char *d_chanid = reinterpret_cast<char *>(info2 + 64);
        if (chanid) HIP_TRY(hipMemcpy(d_chanid, chanid, N, hipMemcpyHostToDevice));
        if (int rc = upload_seq(b, seqnr)) return rc;
        uint32_t raw[4] = {0, 0, 0, 0}, inf[2] = {0, 0};
        HIP_TRY(nmea_format_enqueue(b->ring[0], (int) have, (int) have, b->N, b->d_seq[0], b->d_seq[1], b->d_text,
                                    b->d_text.bytes, b->nmea_scratch, b->nmea_scratch.bytes, raw, nullptr, 0, 0,
                                    nullptr, nullptr));
        HIP_TRY(messages_format_enqueue(b->ring[0], (int) have, b->N, b->d_seq[0], chanid ? d_chanid : nullptr,
                                        b->nmea_scratch, b->nmea_scratch.bytes, lines, len, off, packed,
                                        (size_t) have * line, info2, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(inf, info2, 8, hipMemcpyDeviceToHost));
        if (raw[3]) return fail(GNUAIS_E_HIP, "drain_messages: a frame record names a channel outside the batch");
        const size_t nl = (size_t) raw[0] + raw[1];
        if (nl) HIP_TRY(hipMemcpy(nmea, b->d_text, nl, hipMemcpyDeviceToHost));
        if (inf[0]) HIP_TRY(hipMemcpy(text, packed, inf[0], hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(seqnr, b->d_seq[1], N, hipMemcpyDeviceToHost));
        *nmea_len = nl;
        *text_len = inf[0];
        if (n_sentences) *n_sentences = (int) raw[2];
        if (n_lines) *n_lines = (int) inf[1];
        if (n_frames) *n_frames = (int) have;
    }
    return finish_drain(b, pend, "drain_messages");
}

// Row f3 on the device: what the queued frames do to the reference's position cache, folded per vessel.
// Does not consume the frames (call it before a drain).
int gnuais_batch_fold_vessels(gnuais_batch *b, gnuais_vessel *vessels, int cap, int *n_vessels)
{
    if (!b || !n_vessels || cap < 0 || (cap > 0 && !vessels)) return fail(GNUAIS_E_ARG, "fold_vessels: argument");
    if (b->streaming) return fail(GNUAIS_E_ARG, "fold_vessels: the batch is streaming (gnuais_batch_stream_nmea)");
    *n_vessels = 0;
    Pending pend;
    if (int rc = read_pending(b, pend)) return rc;
    const uint32_t have = pend.have;
    if (!have) return GNUAIS_OK;
    if (int rc = ensure_post_buffers(b, have)) return rc;
    // at most one vessel per frame; the table shares the text buffer (164 bytes per frame >= 120)
    gnuais_vessel *d_tab = reinterpret_cast<gnuais_vessel *>(b->d_text.p);
    const int d_cap = (int) std::min<size_t>(b->d_text.bytes / sizeof(gnuais_vessel), (size_t) have);
    HIP_TRY(b->d_word.ensure(16));
    HIP_TRY(vessels_fold_enqueue(b->ring[0], (int) have, b->nmea_scratch, b->nmea_scratch.bytes, d_tab, d_cap,
                                 b->d_word, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    uint32_t nv = 0;
    HIP_TRY(hipMemcpy(&nv, b->d_word, 4, hipMemcpyDeviceToHost));
    *n_vessels = (int) nv;
    if ((int) nv > cap) return fail(GNUAIS_E_OVERFLOW, "fold_vessels: table too small (*n_vessels entries needed)");
    if (nv) HIP_TRY(hipMemcpy(vessels, d_tab, sizeof(gnuais_vessel) * nv, hipMemcpyDeviceToHost));
    return GNUAIS_OK;
}

// ---- row f3, carried: the position cache kept on the device from batch to batch ------------------------------------
int gnuais_batch_vessel_table_enable(gnuais_batch *b, int capacity)
{
    if (!b || capacity < 1 || capacity > (1 << 24)) return fail(GNUAIS_E_ARG, "vessel_table_enable: capacity 1 .. 2^24");
    if (int rc = gnuais_batch_sync(b)) return rc;
    if (b->s_post) HIP_TRY(hipStreamSynchronize(b->s_post));
    uint32_t slots = 1024;
    while (slots < 2u * (uint32_t) capacity) slots <<= 1;        // at most half full: short probe sequences
    b->vt_slots = 0;
    HIP_TRY(b->vt.alloc(vessel_table_bytes(slots), true));
    HIP_TRY(b->vt_fslot.ensure(sizeof(uint32_t) * (size_t) b->frame_cap));
    b->vt_slots = slots;
    b->vt_capacity = capacity;
    return GNUAIS_OK;
}

int gnuais_batch_vessel_table_clear(gnuais_batch *b)
{
    if (!b || !b->vt) return fail(GNUAIS_E_STATE, "vessel_table_clear: no table (gnuais_batch_vessel_table_enable)");
    if (int rc = gnuais_batch_sync(b)) return rc;
    if (b->s_post) HIP_TRY(hipStreamSynchronize(b->s_post));
    HIP_TRY(hipMemset(b->vt, 0, vessel_table_bytes(b->vt_slots)));
    return GNUAIS_OK;
}

// drain-type use: the queued frames into the table (they stay queued)
int gnuais_batch_vessel_table_update(gnuais_batch *b)
{
    if (!b || !b->vt) return fail(GNUAIS_E_STATE, "vessel_table_update: no table (gnuais_batch_vessel_table_enable)");
    if (b->streaming) return fail(GNUAIS_E_STATE, "vessel_table_update: a streaming batch updates its table by itself");
    if (int rc = discard_flush(b)) return rc;
    if (int rc = gnuais_batch_sync(b)) return rc;             // a drain-type call: waits for the chain like the drains do
    HIP_TRY(vessel_table_update_enqueue(b->ring[0], b->ring_count[0], b->frame_cap, b->vt, b->vt_slots, b->vt_fslot, behind_k3(b)));
    return GNUAIS_OK;
}

int gnuais_batch_vessel_table(gnuais_batch *b, gnuais_vessel *vessels, int cap, int *n_vessels)
{
    if (!b || !n_vessels || cap < 0 || (cap > 0 && !vessels)) return fail(GNUAIS_E_ARG, "vessel_table: argument");
    *n_vessels = 0;
    if (!b->vt) return fail(GNUAIS_E_STATE, "vessel_table: no table (gnuais_batch_vessel_table_enable)");
    if (int rc = set_device(b)) return rc;
    hipStream_t s = b->streaming ? b->s_post : behind_k3(b);
    uint32_t info[4] = {0, 0, 0, 0};
    int n = 0;
    HIP_TRY(vessel_table_fetch(b->vt, b->vt_slots, vessels, cap, &n, info, s));
    *n_vessels = n;
    if (info[1] || (int) info[0] > b->vt_capacity) {
        char msg[160];
        snprintf(msg, sizeof msg, "vessel_table: more vessels than the table was enabled for (%u seen%s, capacity %d)",
                 info[0], info[1] ? ", some dropped" : "", b->vt_capacity);
        return fail(GNUAIS_E_OVERFLOW, msg);
    }
    if (n > cap) return fail(GNUAIS_E_OVERFLOW, "vessel_table: output too small (*n_vessels entries needed)");
    std::sort(vessels, vessels + n, [](const gnuais_vessel &x, const gnuais_vessel &y) { return x.mmsi < y.mmsi; });
    return GNUAIS_OK;
}

int gnuais_batch_drain_frames(gnuais_batch *b, gnuais_frame *h_out, int max, int *n_out)
{
    if (!b || !n_out || (max > 0 && !h_out)) return fail(GNUAIS_E_ARG, "drain_frames: argument");
    *n_out = 0;
    static gnuais_frame none;
    return drain_impl(b, h_out ? h_out : &none, max, n_out, nullptr, nullptr, 0, nullptr, nullptr);
}

// the records and, entry for entry, their receive times (gnuais_batch_frame_times)
int gnuais_batch_drain_frames_timed(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out)
{
    if (!b || !n_out || (max > 0 && (!h_out || !h_times))) return fail(GNUAIS_E_ARG, "drain_frames_timed: argument");
    *n_out = 0;
    if (!b->frame_times) return fail(GNUAIS_E_STATE, "drain_frames_timed: the batch does not time its frames (gnuais_batch_frame_times)");
    static gnuais_frame none;
    static int64_t none_t;
    return drain_impl(b, h_out ? h_out : &none, max, n_out, nullptr, nullptr, 0, nullptr, nullptr, h_times ? h_times : &none_t);
}

// the same with, entry for entry, their power and carrier error (gnuais_batch_frame_signal)
int gnuais_batch_drain_frames_signal(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, gnuais_frame_signal *h_signal,
                                     int max, int *n_out)
{
    if (!b || !n_out || (max > 0 && (!h_out || !h_times || !h_signal))) return fail(GNUAIS_E_ARG, "drain_frames_signal: argument");
    *n_out = 0;
    if (!b->frame_signal) return fail(GNUAIS_E_STATE, "drain_frames_signal: the batch does not measure its frames (gnuais_batch_frame_signal)");
    static gnuais_frame none;
    static int64_t none_t;
    static gnuais_frame_signal none_s;
    return drain_impl(b, h_out ? h_out : &none, max, n_out, nullptr, nullptr, 0, nullptr, nullptr, h_times ? h_times : &none_t,
                      h_signal ? h_signal : &none_s);
}

// The middle of a merging drain, the same for both kinds of frame (frame_unique.hip).  `a` comes with what is the kind's
// own: kind, frames, times, signal, have, and where the output goes on the device (out_first and out_members only where the
// lists are wanted); `name` is the drain's, for the errors.  Here: the scratch and the next tail grow, the hashed attempt,
// then the exact one on the collision word, the range checks, the deliver step, the copies to the host.  The carried
// state -- the tail, the late count -- moves only when everything has succeeded.
static int unique_merge(gnuais_batch *b, gnuais_batch::UniqueState &st, UniqueLaunch &a, const char *name, void *h_out,
                        int64_t *h_times, int32_t *h_copies, int *n_out, int32_t *h_first, gnuais_hearer *h_members,
                        int *n_members)
{
    static_assert(sizeof(gnuais_hearer) == 24 && sizeof(gnuais_frame_signal) == 8, "a member is three 64-bit words");
    const uint32_t have = (uint32_t) a.have;
    const size_t m = (size_t) st.n_tail + have;
    const size_t rec = a.kind == UniqueKind::Long ? sizeof(gnuais_long_frame) : sizeof(gnuais_frame);
    const size_t need = unique_scratch_bytes((int) m, a.kind);
    HIP_TRY(st.scratch.grow(need, need / 4));
    Buf<uint64_t> &next = st.tail[st.cur ^ 1];
    HIP_TRY(next.grow(rec * m, rec * m / 4));
    auto bits_of = [](unsigned long long v) { int n = 1; while (v >> n) ++n; return n; };
    a.tail = st.tail[st.cur];
    a.n_tail = st.n_tail;
    a.tail_out = next;
    a.window = st.window;
    a.rows = (long long) b->rows;
    a.hash_bits = b->uq_hash_bits;
    a.ch_bits = bits_of((unsigned long long) (b->N - 1));
    a.time_bits = bits_of(b->rows);          // t + 1 <= rows
    a.scratch = st.scratch;
    a.scratch_bytes = st.scratch.bytes;
    if (h_first) {
        const size_t need_h = unique_heard_scratch_bytes((int) have);
        HIP_TRY(st.heard.grow(need_h, need_h / 4));
        a.heard_scratch = st.heard;
        a.heard_scratch_bytes = st.heard.bytes;
    }
    uint32_t info[UNIQUE_INFO_WORDS] = {0};
    for (int exact = 0; exact < 2; ++exact) {
        HIP_TRY(unique_cluster_enqueue(a, exact != 0, nullptr));
        HIP_TRY(hipMemcpy(info, unique_info(a.scratch), sizeof info, hipMemcpyDeviceToHost));
        if (!info[UNIQUE_INFO_COLLISION]) break;        // else: two keys share a hash -- once more, by the keys themselves
    }
    const uint32_t np = info[UNIQUE_INFO_PRIMARIES];
    if (np > have || info[UNIQUE_INFO_TAIL] > m)
        return fail(GNUAIS_E_HIP, (std::string(name) + "_unique: the stage's counts are out of range").c_str());
    if (np) {
        HIP_TRY(unique_deliver_enqueue(a, (int) np, nullptr));
        HIP_TRY(hipMemcpy(h_out, a.out_frames, rec * np, hipMemcpyDeviceToHost));
        if (a.out_times) HIP_TRY(hipMemcpy(h_times, a.out_times, sizeof(int64_t) * np, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_copies, a.out_copies, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
        if (h_first) {
            HIP_TRY(hipMemcpy(h_first, a.out_first, sizeof(int32_t) * ((size_t) np + 1), hipMemcpyDeviceToHost));
            const int32_t nm = h_first[np];
            if (nm < 0 || (uint32_t) nm > have)
                return fail(GNUAIS_E_HIP, (std::string(name) + "_heard: the stage's counts are out of range").c_str());
            HIP_TRY(hipMemcpy(h_members, a.out_members, sizeof(gnuais_hearer) * (size_t) nm, hipMemcpyDeviceToHost));
            *n_members = (int) nm;
        }
    }
    unsigned long long late = 0;
    memcpy(&late, info + UNIQUE_INFO_LATE, sizeof late);
    st.cur ^= 1;
    st.n_tail = (int) info[UNIQUE_INFO_TAIL];
    st.late += (long long) late;
    *n_out = (int) np;
    return GNUAIS_OK;
}

// One record per transmission (gnuais_batch_unique): the queued frames and the open clusters of earlier drains go
// through unique_merge; the primaries, their times and the copies cross PCIe once.
// h_first (with h_members and n_members): the clusters' member lists as well (gnuais_batch_drain_frames_heard); the
// launches of a drain without them are what they were.
static int drain_unique_impl(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max, int *n_out,
                             int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    *n_out = 0;
    if (!b->uq.window) return fail(GNUAIS_E_STATE, "drain_frames_unique: the batch does not merge duplicates (gnuais_batch_unique)");
    if (b->streaming) return fail(GNUAIS_E_STATE, "drain_frames_unique: the batch is streaming (gnuais_batch_stream_nmea)");
    Pending pend;
    if (int rc = read_pending(b, pend)) return rc;
    const uint32_t have = pend.have;
    if ((uint32_t) max < have) return fail(GNUAIS_E_ARG, "drain_frames_unique: buffers too small (one entry per pending frame always suffices)");
    if (b->uq.n_tail + have) {                  // without frames the tail still ages
        if (have)
            if (int rc = ensure_post_buffers(b, have)) return rc;
        UniqueLaunch a;
        a.frames = b->ring[0];
        a.times = b->times;
        a.have = (int) have;
        // the text buffer holds 164 bytes per frame: a record, its time and its copies fit side by side
        gnuais_frame *out = reinterpret_cast<gnuais_frame *>(b->d_text.p);
        a.out_frames = out;
        a.out_times = reinterpret_cast<int64_t *>(out + have);
        a.out_copies = reinterpret_cast<int32_t *>(a.out_times + have);
        if (h_first) {
            // ... and behind them the lists: 4 bytes per cluster and one more, 24 per member, 104 * have + 16 in all
            a.signal = b->frame_signal ? b->signal.p : nullptr;
            a.out_first = a.out_copies + have;
            const uintptr_t at = reinterpret_cast<uintptr_t>(a.out_first + have + 1);
            a.out_members = reinterpret_cast<gnuais_hearer *>((at + 15) & ~(uintptr_t) 15);
        }
        if (int rc = unique_merge(b, b->uq, a, "drain_frames", h_out, h_times, h_copies, n_out, h_first, h_members, n_members))
            return rc;
    }
    return finish_drain(b, pend, h_first ? "drain_frames_heard" : "drain_frames_unique", "; results are incomplete");
}

int gnuais_batch_drain_frames_unique(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                     int *n_out)
{
    if (!b || !n_out || max < 0 || (max > 0 && (!h_out || !h_times || !h_copies)))
        return fail(GNUAIS_E_ARG, "drain_frames_unique: argument");
    return drain_unique_impl(b, h_out, h_times, h_copies, max, n_out, nullptr, nullptr, nullptr);
}

// the same drain with, for every cluster, the list of its members: who heard the transmission, when and how strongly
int gnuais_batch_drain_frames_heard(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                    int *n_out, int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    if (!b || !n_out || !n_members || !h_first || max < 0 || (max > 0 && (!h_out || !h_times || !h_copies || !h_members)))
        return fail(GNUAIS_E_ARG, "drain_frames_heard: argument");
    *n_members = 0;
    h_first[0] = 0;
    return drain_unique_impl(b, h_out, h_times, h_copies, max, n_out, h_first, h_members, n_members);
}

// One record per long transmission (gnuais_batch_long_unique): the long ring and the open clusters of earlier drains go
// through unique_merge; the primaries and their copies cross PCIe once.  It ends as the plain long drain ends, by zeroing
// the ring's two words.
// h_first (with h_members and n_members): the clusters' member lists as well (gnuais_batch_drain_long_frames_heard).
static int drain_long_unique_impl(gnuais_batch *b, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out,
                                  int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    const char *who = h_first ? "drain_long_frames_heard" : "drain_long_frames_unique";
    *n_out = 0;
    if (!b->lq.window) return fail(GNUAIS_E_STATE, "drain_long_frames_unique: the batch does not merge long frames (gnuais_batch_long_unique)");
    uint32_t have = 0;
    bool overflow = false;
    if (int rc = long_pending(b, who, have, overflow)) return rc;
    if ((uint32_t) max < have) return fail(GNUAIS_E_ARG, "drain_long_frames_unique: buffers too small (one entry per pending long frame always suffices)");
    if (b->lq.n_tail + have) {                  // without frames the tail still ages
        // the output: records, copies, and for the lists one offset more than records and the members, 8-byte aligned
        const size_t at_copies = sizeof(gnuais_long_frame) * have, at_first = at_copies + 4 * (size_t) have;
        const size_t at_members = (at_first + 4 * ((size_t) have + 1) + 7) & ~(size_t) 7;
        const size_t need_out = at_members + sizeof(gnuais_hearer) * have;
        HIP_TRY(b->lq_out.grow(need_out, need_out / 4));
        UniqueLaunch a;
        a.kind = UniqueKind::Long;
        a.frames = b->long_ring;
        a.have = (int) have;
        a.out_frames = b->lq_out.p;
        a.out_copies = reinterpret_cast<int32_t *>(b->lq_out.p + at_copies);
        if (h_first) {
            a.signal = b->long_frame_signal ? b->long_signal.p : nullptr;
            a.out_first = reinterpret_cast<int32_t *>(b->lq_out.p + at_first);
            a.out_members = reinterpret_cast<gnuais_hearer *>(b->lq_out.p + at_members);
        }
        if (int rc = unique_merge(b, b->lq, a, "drain_long_frames", h_out, nullptr, h_copies, n_out, h_first, h_members, n_members))
            return rc;
    }
    HIP_TRY(hipMemset(b->long_count, 0, sizeof(uint32_t) * 2));
    if (overflow) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: long-frame ring overflowed, frames were dropped", who);
        return fail(GNUAIS_E_OVERFLOW, msg);
    }
    return GNUAIS_OK;
}

int gnuais_batch_drain_long_frames_unique(gnuais_batch *b, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out)
{
    if (!b || !n_out || max < 0 || (max > 0 && (!h_out || !h_copies)))
        return fail(GNUAIS_E_ARG, "drain_long_frames_unique: argument");
    return drain_long_unique_impl(b, h_out, h_copies, max, n_out, nullptr, nullptr, nullptr);
}

// the same drain with, for every cluster, the list of its members: who heard the long transmission, when, and -- while
// gnuais_batch_long_frame_signal is on -- how strongly
int gnuais_batch_drain_long_frames_heard(gnuais_batch *b, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out,
                                         int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    if (!b || !n_out || !n_members || !h_first || max < 0 || (max > 0 && (!h_out || !h_copies || !h_members)))
        return fail(GNUAIS_E_ARG, "drain_long_frames_heard: argument");
    *n_members = 0;
    h_first[0] = 0;
    return drain_long_unique_impl(b, h_out, h_copies, max, n_out, h_first, h_members, n_members);
}

int gnuais_batch_drain_nmea(gnuais_batch *b, uint8_t *seqnr, char *out, size_t out_cap, size_t *out_len,
                            int *n_sentences, int *n_frames)
{
    if (!b || !seqnr || !out_len || (out_cap > 0 && !out)) return fail(GNUAIS_E_ARG, "drain_nmea: argument");
    *out_len = 0;
    if (n_sentences) *n_sentences = 0;
    if (n_frames) *n_frames = 0;
    return drain_impl(b, nullptr, 0, n_frames, seqnr, out, out_cap, out_len, n_sentences);
}

int gnuais_batch_drain_frames_nmea(gnuais_batch *b, gnuais_frame *h_frames, int max, int *n_frames,
                                   uint8_t *seqnr, char *out, size_t out_cap, size_t *out_len, int *n_sentences)
{
    if (!b || !h_frames || !n_frames || !seqnr || !out_len || (out_cap > 0 && !out))
        return fail(GNUAIS_E_ARG, "drain_frames_nmea: argument");
    *n_frames = 0;
    *out_len = 0;
    if (n_sentences) *n_sentences = 0;
    return drain_impl(b, h_frames, max, n_frames, seqnr, out, out_cap, out_len, n_sentences);
}

// First use of the streamed delivery (or back from set_option("streaming", 0)): the other rings, per slot the chunk
// table, texts and events, the info words, the copy stream, the carried sequence digits.
static int stream_setup(gnuais_batch *b)
{
    constexpr int NR = gnuais_batch::NRING;
    const size_t N = (size_t) b->N;
    const size_t text_cap = (size_t) b->frame_cap * 164;        // a full ring of two-sentence frames
    if (b->frame_times) return fail(GNUAIS_E_STATE, "stream_nmea: the batch times its frames (gnuais_batch_frame_times); "
                                                    "the streamed delivery carries no times");
    if (b->repair) return fail(GNUAIS_E_STATE, "stream_nmea: the batch repairs frames (gnuais_batch_repair); the streamed "
                                               "delivery's order table describes the CRC stage's records only");
    if (b->frame_signal) return fail(GNUAIS_E_STATE, "stream_nmea: the batch measures its frames (gnuais_batch_frame_signal); "
                                                     "the streamed delivery carries no records of them");
    if (b->uq.window) return fail(GNUAIS_E_STATE, "stream_nmea: the batch merges duplicates (gnuais_batch_unique); the "
                                                  "streamed delivery has no such stage");
    if (b->long_frames) return fail(GNUAIS_E_STATE, "stream_nmea: the batch decodes long frames (gnuais_batch_long_frames); "
                                                    "the streamed delivery carries no records of them");
    if (int rc = discard_flush(b)) return rc;   // ring 0 is about to be handed to the streamed delivery
    if (int rc = gnuais_batch_sync(b)) return rc;
    // every object is created only if it does not exist yet: a first use that failed half way (e.g. the pinned
    // allocation) is repeated by the next call without leaking what the failed one had made
    for (int q = 1; q < NR; ++q) {
        HIP_TRY(b->ring[q].ensure(sizeof(gnuais_frame) * (size_t) b->frame_cap));
        HIP_TRY(b->ring_count[q].ensure(sizeof(uint32_t) * 4, true));
    }
    b->n_chunks = k3_blocks(b->N) * k3_passes(b->cand_K);
    b->sh_text_want = std::max(b->sh_text_want, ((size_t) b->frame_cap * 32 + 65536) & ~(size_t) 15);
    for (int q = 0; q < NR; ++q) {
        HIP_TRY(b->ring_chunks[q].ensure(sizeof(uint2) * (size_t) b->n_chunks));
        b->ring_runs[q] = 2;                // whatever ring 0 holds by now came without a table
        HIP_TRY(b->sd_text[q].ensure(text_cap));
        for (Event *e : {&b->e_fill[q], &b->e_fmt[q], &b->e_txt[q]}) HIP_TRY(e->ensure(hipEventDisableTiming));
        // pinned text: a fifth of the worst case to begin with (single-sentence frames of average
        // length fill it to about a third); a slot whose text does not fit grows, see (3)
        HIP_TRY(b->sh_text[q].ensure(b->sh_text_want));
    }
    HIP_TRY(b->sd_info.ensure(sizeof(uint32_t) * 8 * NR, true));
    if (const char *v = getenv("GNUAIS_COPY_WGS")) b->copy_wgs = std::max(1, atoi(v));
    if (const char *v = getenv("GNUAIS_COPY_ON_K3")) b->copy_on_k3 = atoi(v) != 0;
    HIP_TRY(b->nmea_scratch.grow(nmea_scratch_bytes(b->frame_cap, b->n_chunks)));
    if (!b->s_copy_own) {
        // The formatter's kernels go onto K3's stream: they are small, K3's stream is idle most of a call,
        // and every further stream is one more tenant for the few hardware queues (a formatter stream
        // that shares its queue with a stage serialises with it: 0.8 or 1.5 ms per call, by luck).
        // Only the copy, which lasts as long as PCIe needs, has a stream of its own.
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(b->s_copy_own.ensure(hi));
        b->s_copy = b->s_copy_own;
    }
    HIP_TRY(b->sh_info.ensure(sizeof(uint32_t) * 8 * NR, true));
    for (auto &p : b->sd_seq) HIP_TRY(p.ensure(N, true));
    HIP_TRY(hipDeviceSynchronize());
    b->streaming = true;
    return GNUAIS_OK;
}

// Streaming delivery (row f1 end to end).  Call after every gnuais_batch_run(): the frames of the
// runs since the previous call are taken off (K3 moves on to the next ring at once) and go through
// three later calls -- two calls on: count read + device formatter queued; then: text copy into pinned
// memory queued; then: text handed out -- so that no call waits for work queued in the same call.
int gnuais_batch_stream_nmea(gnuais_batch *b, const char **text, size_t *len, int *n_sentences, int *n_frames)
{
    if (!b || !text || !len) return fail(GNUAIS_E_ARG, "stream_nmea: argument");
    if (int rc = set_device(b)) return rc;
    *text = nullptr;
    *len = 0;
    if (n_sentences) *n_sentences = 0;
    if (n_frames) *n_frames = -1;               // nothing handed out yet
    constexpr int NR = gnuais_batch::NRING;
    const size_t N = (size_t) b->N;
    if (!b->streaming)
        if (int rc = stream_setup(b)) return rc;
    hipStream_t sD = behind_k3(b);
    const int c = b->ring_cur;
    // (1) ring c: everything K3 has been asked to append so far
    HIP_TRY(hipEventRecord(b->e_fill[c], sD));
    const int runs = b->ring_runs[c];
    // (2) K3 moves on to the next ring; that ring's formatter (queued NRING - 1 calls ago) must be done
    const int nx = (c + 1) % NR;
    if (b->s_stage[nx]) HIP_TRY(hipStreamWaitEvent(sD, b->e_fmt[nx], 0));
    b->ring_cur = nx;
    b->ring_runs[nx] = 0;
    // (3) hand out the text of slot nx, queued NRING - 1 calls ago: the only wait of this call.  (Before (4): a slow-path copy below must not queue behind it.)
    int rc_late = GNUAIS_OK;
    if (b->s_stage[nx]) {
        HIP_TRY(hipEventSynchronize(b->e_txt[nx]));
        const uint32_t *info = b->sh_info + 8 * nx;
        const uint32_t have = std::min<uint32_t>(info[4], (uint32_t) b->frame_cap);
        const size_t n_text = (size_t) info[0] + info[1];
        if (n_text > b->sh_text[nx].bytes) {
            // the pinned buffer was too small for this slot (the first calls, or traffic grew): make it larger
            // and fetch the text from the device copy, which stays intact until the slot is formatted again
            const size_t want = std::max(b->sh_text_want, (n_text + n_text / 2 + 65536) & ~(size_t) 15);
            b->sh_text_want = want;
            HIP_TRY(b->sh_text[nx].grow(b->sh_text_want));
            HIP_TRY(hipMemcpyAsync(b->sh_text[nx], b->sd_text[nx], n_text, hipMemcpyDeviceToHost, b->s_copy));
            HIP_TRY(hipStreamSynchronize(b->s_copy));
        }
        *text = b->sh_text[nx];
        *len = n_text;
        if (n_sentences) *n_sentences = (int) info[2];
        if (n_frames) *n_frames = (int) have;
        b->s_stage[nx] = 0;
        if (info[3]) rc_late = fail(GNUAIS_E_HIP, "stream_nmea: a frame record names a channel outside the batch");
        else rc_late = late_error("stream_nmea", info[7] != 0, info[5] || info[4] > (uint32_t) b->frame_cap);
    }
    // (4) ring c: order, sequence digits, text, copy into pinned memory -- queued now, behind its K3, with
    // every size taken on the device
    b->s_post = sD;                             // behind the K3 launches that filled the ring, in stream order
    uint32_t *totals = nullptr;
    HIP_TRY(b->sh_text[c].grow(b->sh_text_want));               // catch up with a buffer that had to grow (slot c is idle)
    if (runs >= 1) {
        int n_host = -1;                        // one run: K3's chunk table is the order, the count stays on the device
        if (runs > 1) {                         // several runs share the ring: count on the host, radix sort
            uint32_t cnt[4];
            HIP_TRY(hipStreamSynchronize(b->s_post));
            HIP_TRY(hipMemcpy(cnt, b->ring_count[c], 16, hipMemcpyDeviceToHost));
            n_host = (int) std::min<uint32_t>(cnt[0], (uint32_t) b->frame_cap);
        }
        if (n_host != 0) {
            uint8_t *sin = b->sd_seq[b->sd_seq_cur], *sout = b->sd_seq[b->sd_seq_cur ^ 1];
            HIP_TRY(hipMemcpyAsync(sout, sin, N, hipMemcpyDeviceToDevice, b->s_post));
            HIP_TRY(nmea_format_enqueue(b->ring[c], n_host, b->frame_cap, b->N, sin, sout, b->sd_text[c],
                                        b->sd_text[c].bytes, b->nmea_scratch, b->nmea_scratch.bytes, nullptr,
                                        b->ring_chunks[c], b->n_chunks, k3_passes(b->cand_K), &totals, b->s_post));
            b->sd_seq_cur ^= 1;
        }
    }
    // the span's frames into the carried vessel table, behind the formatter and before the ring is handed back
    if (b->vt && runs >= 1)
        HIP_TRY(vessel_table_update_enqueue(b->ring[c], b->ring_count[c], b->frame_cap, b->vt, b->vt_slots, b->vt_fslot,
                                            b->s_post));
    HIP_TRY(nmea_slot_info_enqueue(totals, b->ring_count[c], b->sd_info + 8 * c, b->s_post));
    HIP_TRY(hipMemsetAsync(b->ring_count[c], 0, 16, b->s_post));
    HIP_TRY(hipEventRecord(b->e_fmt[c], b->s_post));          // the ring is free for K3 again
    // (5) the copy has a stream of its own: it runs at PCIe speed beside the next slot's formatter
    hipStream_t sc = b->copy_on_k3 ? b->s_post : b->s_copy;
    if (!b->copy_on_k3) HIP_TRY(hipStreamWaitEvent(sc, b->e_fmt[c], 0));
    HIP_TRY(nmea_text_copy_enqueue(b->sd_text[c], b->sd_info + 8 * c, b->sh_text[c], b->sh_text[c].bytes,
                                   b->sh_info + 8 * c, b->copy_wgs, sc));
    HIP_TRY(hipEventRecord(b->e_txt[c], sc));
    b->s_stage[c] = 1;
    b->hdlc_calls = 0;
    b->stream_calls++;
    return rc_late;
}

int gnuais_batch_pending_frames(gnuais_batch *b, int *n_out)
{
    if (!b || !n_out) return fail(GNUAIS_E_ARG, "pending_frames: argument");
    if (b->streaming) return fail(GNUAIS_E_STATE, "pending_frames: the batch is streaming (gnuais_batch_stream_nmea)");
    Pending pend;
    if (int rc = read_pending(b, pend)) return rc;
    *n_out = (int) pend.have;
    return GNUAIS_OK;
}

int gnuais_batch_discard_frames(gnuais_batch *b, void *stream)
{
    if (!b) return fail(GNUAIS_E_ARG, "discard_frames: NULL batch");
    if (b->streaming) return fail(GNUAIS_E_STATE, "discard_frames: the batch is streaming (gnuais_batch_stream_nmea)");
    if (int rc = set_device(b)) return rc;
    // Behind the last K3, in stream order.  No dispatch for it: the next deframer launch runs exactly there -- behind the
    // previous K3, in front of its own -- and empties the ring's words itself (HdlcLaunch::discard); whoever looks at the
    // ring before that launch turns the mark into the memset first (discard_flush).  Two discards in a row are one.
    b->discard_stream = (hipStream_t) stream;   // where the chain runs when it is not pipelined
    b->discard_pending = true;
    if (!(b->cycle_parts & 1))
        if (int rc = discard_flush(b)) return rc;
    b->hdlc_calls = 0;
    return GNUAIS_OK;
}

// The delivery loop (run + stream_nmea) has one more stream to place: the copy kernel's.  Which hardware
// queue a stream shares is not queryable (see gnuais_batch_autotune); a copy stream that shares its queue with
// a stage serialises with it (0.62 against 1.5 ms per C3 call).  Times the loop with the copy kernel on each
// free pool stream and on the stream created for it, keeps the fastest, resets the batch (it stays in
// streaming mode).
int gnuais_batch_autotune_delivery(gnuais_batch *b, const int16_t *d_samples, int len, void *stream, float *ms_per_call)
{
    if (!b || !d_samples) return fail(GNUAIS_E_ARG, "autotune_delivery: NULL argument");
    if (int rc = gnuais_batch_sync(b)) return rc;
    const char *text = nullptr;
    size_t tl = 0;
    if (int rc = gnuais_batch_stream_nmea(b, &text, &tl, nullptr, nullptr)) return rc;      // rings, buffers, s_copy
    if (!b->pipeline) {
        if (ms_per_call) *ms_per_call = 0.0f;
        return gnuais_batch_reset(b);
    }
    const bool timing = b->timing;
    b->timing = false;
    auto quiesce = [&]() -> int {
        if (int rc = gnuais_batch_sync(b)) return rc;
        HIP_TRY(hipDeviceSynchronize());
        return GNUAIS_OK;
    };
    auto measure = [&](double &ms, int meas) -> int {
        const int warm = gnuais_batch::NRING + 2;
        for (int i = 0; i < warm + meas; ++i) {
            if (i == warm) {
                if (int rc = quiesce()) return rc;
                ms = -now_ms();
            }
            if (int rc = gnuais_batch_run(b, d_samples, len, stream)) return rc;
            const int rc = gnuais_batch_stream_nmea(b, &text, &tl, nullptr, nullptr);
            if (rc != GNUAIS_OK && rc != GNUAIS_E_OVERFLOW) return rc;
        }
        if (int rc = quiesce()) return rc;
        ms = (ms + now_ms()) / meas;
        return GNUAIS_OK;
    };
    hipStream_t own = b->s_copy_own;
    // twelve calls per candidate, then the two fastest again over thirty (a dozen calls are noisy)
    hipStream_t top[2] = {own, own};
    double top_ms[2] = {1e30, 1e30};
    for (int cand = -1; cand < gnuais_batch::POOL; ++cand) {
        hipStream_t st = cand < 0 ? own : b->pool[cand];
        bool used = false;
        for (int q = 0; q < 4; ++q) used |= b->s_k[q] == st;
        if (used || !st) continue;
        b->s_copy = st;
        double ms = 0;
        if (int rc = measure(ms, 12)) return rc;
        if (ms < top_ms[0]) { top_ms[1] = top_ms[0]; top[1] = top[0]; top_ms[0] = ms; top[0] = st; }
        else if (ms < top_ms[1]) { top_ms[1] = ms; top[1] = st; }
    }
    hipStream_t best_s = top[0];
    double best = 1e30;
    for (int k = 0; k < 2; ++k) {
        if (k == 1 && top[1] == top[0]) break;
        b->s_copy = top[k];
        double ms = 0;
        if (int rc = measure(ms, 30)) return rc;
        if (ms < best) { best = ms; best_s = top[k]; }
    }
    b->s_copy = best_s;
    b->timing = timing;
    if (ms_per_call) *ms_per_call = (float) best;
    return gnuais_batch_reset(b);
}

} // extern "C"
