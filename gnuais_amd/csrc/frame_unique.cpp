// frame_unique.cpp -- gnuais_uniq and gnuais_long_uniq: the duplicate merge of the definition in include/gnuais_hip.h
// (gnuais_batch_unique, gnuais_batch_long_unique) on the host, one drain per push.  One statement, push_impl, over the
// kind of record (frame_unique.h: ShortRec, LongRec).  It is the exact statement the device stage (frame_unique.hip over
// ShortDev and LongDev) must equal bit for bit, and what a node runs over the merged drains of its shards.  Plain C++,
// no HIP.
#include "frame_unique.h"

#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/gnuais_hip.h"

using namespace gnuais::uniq;

namespace {

// the record kinds as the host sees them: the public struct, and where a frame's time comes from
struct ShortHost : ShortRec {
    typedef gnuais_frame Frame;
    static long long time_of(const Frame &, const int64_t *times, int i) { return times[i]; }
};
struct LongHost : LongRec {
    typedef gnuais_long_frame Frame;
    static long long time_of(const Frame &f, const int64_t *, int) { return f.t; }
};
static_assert(sizeof(gnuais_frame) == 4 * ShortRec::REC_WORDS && sizeof(gnuais_long_frame) == 4 * LongRec::REC_WORDS,
              "the traits' record sizes");

template <class R> struct Key {
    uint32_t w[R::KEY_WORDS];
    bool operator==(const Key &o) const { return memcmp(w, o.w, sizeof w) == 0; }
    bool operator<(const Key &o) const { return memcmp(w, o.w, sizeof w) < 0; }
};

template <class R> struct Tail {
    Key<R> key;
    long long t_last;
};

// a member of the sort: a tail entry (src < 0) or frame `src` of the push
template <class R> struct Member {
    Key<R> key;
    long long t;
    uint32_t channel;
    int src;
};

// the output order: the untimed frames (t = -1) first, by (channel, stamp) as the plain drain orders them, then the timed
// ones by (t, channel).  t is compared as it is, not packed into output_word(): that word holds rows below 2^39 only.
struct Primary {
    long long t;
    uint64_t order;             // untimed: output_word(); timed: the channel
    int src, copies;
    size_t start;               // its members: mem[start .. start + copies) of the sort, unused for an untimed frame
};

template <class R> void words_of(const typename R::Frame &f, uint32_t rec[R::REC_WORDS]) { memcpy(rec, &f, 4 * R::REC_WORDS); }

template <class R> Key<R> key_of(const typename R::Frame &f)
{
    uint32_t rec[R::REC_WORDS];
    words_of<R>(f, rec);
    Key<R> k;
    for (int i = 0; i < R::KEY_WORDS; ++i) k.w[i] = R::key_word(rec, i);
    return k;
}

// the carried state of one merge object
template <class R> struct State {
    long long window = 0, late = 0;
    std::vector<Tail<R>> tail;
};

} // namespace

struct gnuais_uniq : State<ShortHost> {};
struct gnuais_long_uniq : State<LongHost> {};

namespace {

template <class U> int create(U **out, long long window)
{
    if (!out) return GNUAIS_E_ARG;
    *out = nullptr;
    if (window <= 0) return GNUAIS_E_ARG;
    U *u = new (std::nothrow) U;
    if (!u) return GNUAIS_E_ARG;
    u->window = window;
    *out = u;
    return GNUAIS_OK;
}

template <class U> int reset(U *u)
{
    if (!u) return GNUAIS_E_ARG;
    u->tail.clear();
    u->late = 0;
    return GNUAIS_OK;
}

template <class R>
gnuais_hearer hearer_of(const typename R::Frame &f, long long t, const gnuais_frame_signal *signal)
{
    uint32_t rec[R::REC_WORDS];
    words_of<R>(f, rec);
    gnuais_hearer h;
    h.channel = f.channel;
    h.flags = R::flags(rec);
    h.t = t < 0 ? -1 : t;
    h.signal = signal ? *signal : gnuais_frame_signal{0, 0, 0};
    return h;
}

// one drain of the definition; with out_first the member lists of gnuais_batch_drain_frames_heard as well.  Where the
// record carries its own time (R::TIMED_BY_RECORD) times and out_times are not read or written.
template <class R>
int push_impl(State<R> *u, const typename R::Frame *frames, const int64_t *times, const gnuais_frame_signal *signal, int n,
              long long rows, typename R::Frame *out, int64_t *out_times, int32_t *out_copies, int cap, int *n_out,
              int32_t *out_first, gnuais_hearer *out_members, int *n_members)
{
    constexpr bool own_t = R::TIMED_BY_RECORD;
    if (!u || !n_out || n < 0 || cap < 0 || rows < 0 || (n > 0 && (!frames || (!own_t && !times))) ||
        (cap > 0 && (!out || (!own_t && !out_times) || !out_copies)))
        return GNUAIS_E_ARG;
    *n_out = 0;
    const long long W = u->window;
    std::vector<Member<R>> mem;
    std::vector<Primary> prim;
    mem.reserve(u->tail.size() + (size_t) n);
    for (const Tail<R> &t : u->tail) mem.push_back(Member<R>{t.key, t.t_last, 0u, -1});
    for (int i = 0; i < n; ++i) {
        const long long t = R::time_of(frames[i], times, i);
        if (t < 0) {                    // untimed: a cluster by itself
            uint32_t rec[R::REC_WORDS];
            words_of<R>(frames[i], rec);
            prim.push_back(Primary{-1, output_word(-1, frames[i].channel, R::stamp37(rec)), i, 1, 0});
        } else {
            mem.push_back(Member<R>{key_of<R>(frames[i]), t, frames[i].channel, i});
        }
    }
    // key, then the member order (t, channel); a tail entry lies before every frame of this push (t_last < rows <= t)
    std::sort(mem.begin(), mem.end(), [](const Member<R> &a, const Member<R> &b) {
        if (!(a.key == b.key)) return a.key < b.key;
        if (a.t != b.t) return a.t < b.t;
        if ((a.src < 0) != (b.src < 0)) return a.src < 0;
        return a.channel < b.channel;
    });
    std::vector<Tail<R>> tail;
    long long late = 0;
    for (size_t s = 0; s < mem.size();) {
        size_t e = s + 1;
        while (e < mem.size() && mem[e].key == mem[s].key && mem[e].t - mem[e - 1].t <= W) ++e;
        const bool from_tail = mem[s].src < 0;
        const int size = (int) (e - s) - (from_tail ? 1 : 0);
        if (from_tail) {
            late += size;               // copies of a transmission an earlier push delivered
        } else {
            // the first member in (repaired, t, channel): the earliest intact one, else the earliest
            size_t p = s;
            for (size_t j = s; j < e; ++j) {
                uint32_t rec[R::REC_WORDS];
                words_of<R>(frames[mem[j].src], rec);
                if (!R::repaired_bit(rec)) { p = j; break; }
            }
            prim.push_back(Primary{mem[p].t, mem[p].channel, mem[p].src, size, s});
        }
        if (mem[e - 1].t + W >= rows) tail.push_back(Tail<R>{mem[s].key, mem[e - 1].t});
        s = e;
    }
    if (prim.size() > (size_t) cap) return GNUAIS_E_ARG;        // nothing consumed: tail and late are as they were
    std::sort(prim.begin(), prim.end(), [](const Primary &a, const Primary &b) {
        if (a.t != b.t) return a.t < b.t;
        return a.order != b.order ? a.order < b.order : a.src < b.src;
    });
    for (size_t j = 0; j < prim.size(); ++j) {
        out[j] = frames[prim[j].src];
        if (!own_t) out_times[j] = times[prim[j].src];
        out_copies[j] = prim[j].copies;
    }
    if (out_first) {
        // the members of a cluster lie together in the sort, in member order (t, channel); late ones are listed nowhere
        int32_t at = 0;
        out_first[0] = 0;
        for (size_t j = 0; j < prim.size(); ++j) {
            const Primary &p = prim[j];
            if (p.t < 0) {
                out_members[at++] = hearer_of<R>(frames[p.src], -1, signal ? signal + p.src : nullptr);
            } else {
                for (size_t k = p.start; k < p.start + (size_t) p.copies; ++k)
                    out_members[at++] = hearer_of<R>(frames[mem[k].src], mem[k].t, signal ? signal + mem[k].src : nullptr);
            }
            out_first[j + 1] = at;
        }
        *n_members = (int) at;
    }
    u->tail.swap(tail);
    u->late += late;
    *n_out = (int) prim.size();
    return GNUAIS_OK;
}

} // namespace

extern "C" {

int gnuais_uniq_create(gnuais_uniq **out, long long window) { return create(out, window); }
void gnuais_uniq_destroy(gnuais_uniq *u) { delete u; }
int gnuais_uniq_reset(gnuais_uniq *u) { return reset(u); }
long long gnuais_uniq_late(const gnuais_uniq *u) { return u ? u->late : 0; }

int gnuais_uniq_push(gnuais_uniq *u, const gnuais_frame *frames, const int64_t *times, int n, long long rows,
                     gnuais_frame *out, int64_t *out_times, int32_t *out_copies, int cap, int *n_out)
{
    return push_impl<ShortHost>(u, frames, times, nullptr, n, rows, out, out_times, out_copies, cap, n_out, nullptr, nullptr,
                                nullptr);
}

int gnuais_uniq_push_heard(gnuais_uniq *u, const gnuais_frame *frames, const int64_t *times, const gnuais_frame_signal *signal,
                           int n, long long rows, gnuais_frame *out, int64_t *out_times, int32_t *out_copies, int cap,
                           int *n_out, int32_t *out_first, gnuais_hearer *out_members, int *n_members)
{
    if (!out_first || !n_members || (n > 0 && !out_members)) return GNUAIS_E_ARG;
    *n_members = 0;
    out_first[0] = 0;
    return push_impl<ShortHost>(u, frames, times, signal, n, rows, out, out_times, out_copies, cap, n_out, out_first,
                                out_members, n_members);
}

// the long frames' merge: the time is the record's own t; the members carry the records of _push_heard_signal, else zeros
int gnuais_long_uniq_create(gnuais_long_uniq **out, long long window) { return create(out, window); }
void gnuais_long_uniq_destroy(gnuais_long_uniq *u) { delete u; }
int gnuais_long_uniq_reset(gnuais_long_uniq *u) { return reset(u); }
long long gnuais_long_uniq_late(const gnuais_long_uniq *u) { return u ? u->late : 0; }

int gnuais_long_uniq_push(gnuais_long_uniq *u, const gnuais_long_frame *frames, int n, long long rows,
                          gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out)
{
    return push_impl<LongHost>(u, frames, nullptr, nullptr, n, rows, out, nullptr, out_copies, cap, n_out, nullptr, nullptr,
                               nullptr);
}

int gnuais_long_uniq_push_heard(gnuais_long_uniq *u, const gnuais_long_frame *frames, int n, long long rows,
                                gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out, int32_t *out_first,
                                gnuais_hearer *out_members, int *n_members)
{
    if (!out_first || !n_members || (n > 0 && !out_members)) return GNUAIS_E_ARG;
    *n_members = 0;
    out_first[0] = 0;
    return push_impl<LongHost>(u, frames, nullptr, nullptr, n, rows, out, nullptr, out_copies, cap, n_out, out_first,
                               out_members, n_members);
}

int gnuais_long_uniq_push_heard_signal(gnuais_long_uniq *u, const gnuais_long_frame *frames, const gnuais_frame_signal *signal,
                                       int n, long long rows, gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out,
                                       int32_t *out_first, gnuais_hearer *out_members, int *n_members)
{
    if (!out_first || !n_members || (n > 0 && !out_members)) return GNUAIS_E_ARG;
    *n_members = 0;
    out_first[0] = 0;
    return push_impl<LongHost>(u, frames, nullptr, signal, n, rows, out, nullptr, out_copies, cap, n_out, out_first,
                               out_members, n_members);
}

} // extern "C"
