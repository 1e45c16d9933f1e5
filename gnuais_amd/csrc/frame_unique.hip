// frame_unique.hip -- the duplicate merge on the device, for the short and the long frames (definition:
// include/gnuais_hip.h, gnuais_batch_unique and gnuais_batch_long_unique; the host statement it must equal bit for bit:
// frame_unique.cpp).
//
// Nothing runs per call: the whole stage is the drain.  Entries are [tail | ring]: the open clusters an earlier drain
// left behind and the frames the deframer appended.  Lane = entry (or sorted position, or cluster) in every kernel; no
// LDS, no scratch memory.  One text serves both kinds of record: every kernel but slot2q is a template over a record
// policy, ShortDev or LongDev (frame_unique_dev.h), which says how a record, its key, its time and a list member are
// read and written -- 16-byte quarters and a times array beside the ring for the one, 64-bit words and the record's own
// time for the other.  PAIRS below is 7 / 17, the key as 64-bit digits.
//
//   keys      per entry: the member-order word (t + 1) << ch_bits | channel and a 64-bit hash of the key
//   sort      stable radix sort by the order word, then by the hash: every key's entries lie together in member order
//   digit     per sorted position: the hash, or one pair of key words, of the entry there: the next stable sort's digit
//   boundary  per position: is the neighbour before it the same key (hash AND every key word) and within the window?
//             Equal hashes with unequal keys raise the collision flag: the caller then repeats the sort in its exact
//             form -- PAIRS stable sorts by the key words themselves in place of the one by the hash -- so the result
//             never depends on the hash (set_option("unique_hash_bits") truncates it for the tests).
//   scan      cluster number of every position (inclusive sum of the head flags)
//   members   per position: the cluster's start, and an atomic minimum of (repaired, position) over its frames -- the
//             primary; a minimum does not depend on arrival order, and a cluster may be any size
//   clusters  per cluster: copies, late copies (behind a tail entry), the primary into a compacted list with its output
//             order word, the cluster into the next tail if its last member is within the window of `rows`: the short
//             kind writes the 64-byte entry from registers; the long kind (TAIL_BY_WORDS) notes the entry and t_last
//   tail      long kind only, thread = (tail slot, 64-bit word): the noted entry into the next tail, adjacent lanes on
//             adjacent words
//   deliver   sort of the primaries by the output word (unique per record, so the slot order of the compaction does
//             not show), gather with thread = (record, quarter or 64-bit word) of records, times and copies: 76 bytes
//             per delivered short frame cross PCIe, 156 per long one
//   heard     only where the member lists are wanted (gnuais_batch_drain_frames_heard, _long_frames_heard): scan of the
//             copies in output order = the lists' offsets, a map from a primary's ring slot to its output position, and
//             per sorted position the member's 24 bytes into its cluster's list (a cluster's members lie together in the
//             sort)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "frame_unique_dev.h"
#include "kernels.h"

namespace gnuais {

namespace {

constexpr int BLOCK = 256;

// the scratch of one drain of m entries, 256-byte slots; tsrc and tlast only where the tail kernel runs
struct Layout {
    uint32_t *info;             // UNIQUE_INFO_WORDS
    u64 *tw, *hash, *kA, *kB, *prim, *tlast;
    uint32_t *idxA, *idxB, *head, *cid, *start, *pent, *pidx, *pidx2, *tsrc;
    int32_t *pcopies;
    void *tmp;
    size_t tmp_bytes;
};

size_t rocprim_tmp_bytes(size_t m)
{
    size_t sort_tmp = 0, scan_tmp = 0;
    (void) rocprim::radix_sort_pairs(nullptr, sort_tmp, (u64 *) nullptr, (u64 *) nullptr, (uint32_t *) nullptr,
                                     (uint32_t *) nullptr, m, 0, 64, (hipStream_t) 0);
    (void) rocprim::inclusive_scan(nullptr, scan_tmp, (uint32_t *) nullptr, (uint32_t *) nullptr, m,
                                   rocprim::plus<uint32_t>(), (hipStream_t) 0);
    return sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
}

inline size_t slot(size_t bytes) { return (bytes + 255) / 256 * 256; }

Layout carve(void *scratch, size_t scratch_bytes, size_t m, bool tail_by_words)
{
    char *p = static_cast<char *>(scratch);
    auto take = [&](size_t bytes) { char *q = p; p += slot(bytes); return (void *) q; };
    Layout l;
    l.info = (uint32_t *) take(4 * UNIQUE_INFO_WORDS);
    l.tw = (u64 *) take(8 * m);
    l.hash = (u64 *) take(8 * m);
    l.kA = (u64 *) take(8 * m);
    l.kB = (u64 *) take(8 * m);
    l.prim = (u64 *) take(8 * m);
    l.tlast = tail_by_words ? (u64 *) take(8 * m) : nullptr;
    l.idxA = (uint32_t *) take(4 * m);
    l.idxB = (uint32_t *) take(4 * m);
    l.head = (uint32_t *) take(4 * m);
    l.cid = (uint32_t *) take(4 * m);
    l.start = (uint32_t *) take(4 * (m + 1));
    l.pent = (uint32_t *) take(4 * m);
    l.pidx = (uint32_t *) take(4 * m);
    l.pidx2 = (uint32_t *) take(4 * m);
    l.tsrc = tail_by_words ? (uint32_t *) take(4 * m) : nullptr;
    l.pcopies = (int32_t *) take(4 * m);
    l.tmp = p;
    l.tmp_bytes = scratch_bytes - (size_t) (p - static_cast<char *>(scratch));
    return l;
}

// entry i of [tail | ring]: its words
template <class R>
__device__ __forceinline__ const typename R::word *entry_rec(const typename R::word *tail, int n_tail,
                                                             const typename R::word *frames, uint32_t i)
{
    return i < (uint32_t) n_tail ? tail + (size_t) i * R::WORDS : frames + (size_t) (i - (uint32_t) n_tail) * R::WORDS;
}

template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_keys_kernel(
    const typename R::word *__restrict__ tail, int n_tail, const typename R::word *__restrict__ frames,
    const long long *__restrict__ times, int m, int ch_bits, int hash_bits, u64 *__restrict__ tw,
    u64 *__restrict__ hash, uint32_t *__restrict__ idx, u64 *__restrict__ prim)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const typename R::Image r = R::load(entry_rec<R>(tail, n_tail, frames, (uint32_t) i));
    long long t;
    uint32_t ch = 0;
    if (i < n_tail) {
        t = R::tail_time(r.w);
    } else {
        t = R::frame_time(r.w, times, (uint32_t) (i - n_tail));
        if (t < -1) t = -1;
        ch = R::channel(r.w);
    }
    u64 h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int p = 0; p < R::PAIRS; ++p) {
        h ^= R::pair(r.w, p);
        h *= 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 29;
    tw[i] = ((u64) (t + 1) << ch_bits) | (u64) ch;
    hash[i] = h >> (64 - hash_bits);
    idx[i] = (uint32_t) i;
    prim[i] = ~0ull;
}

// the hash, or one pair of key words, of the entries in their current order: the next stable sort's digit
template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_digit_kernel(
    const typename R::word *__restrict__ tail, int n_tail, const typename R::word *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ hash, int pair, u64 *__restrict__ out)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t e = idx[j];
    out[j] = pair < 0 ? hash[e] : R::pair(entry_rec<R>(tail, n_tail, frames, e), pair);
}

template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_boundary_kernel(
    const typename R::word *__restrict__ tail, int n_tail, const typename R::word *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ hs, const u64 *__restrict__ tw, int ch_bits,
    long long window, int exact, uint32_t *__restrict__ head, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    uint32_t is_head = 1;
    if (j > 0 && (exact || hs[j] == hs[j - 1])) {
        const uint32_t e = idx[j], p = idx[j - 1];
        const typename R::Image a = R::load(entry_rec<R>(tail, n_tail, frames, e));
        const typename R::Image b = R::load(entry_rec<R>(tail, n_tail, frames, p));
        u64 diff = 0;
#pragma unroll
        for (int k = 0; k < R::PAIRS; ++k) diff |= R::pair(a.w, k) ^ R::pair(b.w, k);
        if (diff) {
            if (!exact) info[UNIQUE_INFO_COLLISION] = 1u;      // every writer writes the same word
        } else {
            const long long te = (long long) (tw[e] >> ch_bits) - 1, tp = (long long) (tw[p] >> ch_bits) - 1;
            if (te >= 0 && tp >= 0 && te - tp <= window) is_head = 0;
        }
    }
    head[j] = is_head;
}

template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_members_kernel(
    int n_tail, const typename R::word *__restrict__ frames, int m, const uint32_t *__restrict__ idx,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ cid, uint32_t *__restrict__ start,
    u64 *__restrict__ prim, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u;             // cid is an inclusive sum that starts with a head: >= 1
    if (head[j]) start[c] = (uint32_t) j;
    if (j == m - 1) {
        start[c + 1] = (uint32_t) m;
        info[UNIQUE_INFO_CLUSTERS] = c + 1u;
    }
    const uint32_t e = idx[j];
    if (e >= (uint32_t) n_tail) {
        const typename R::word *rec = frames + (size_t) (e - (uint32_t) n_tail) * R::WORDS;
        atomicMin(&prim[c], ((u64) R::repaired_bit(rec) << 32) | (u64) (uint32_t) j);
    }
}

template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_clusters_kernel(
    const typename R::word *__restrict__ tail, int n_tail, const typename R::word *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ tw, int ch_bits, long long window, long long rows,
    const uint32_t *__restrict__ start, const u64 *__restrict__ prim, uint32_t *__restrict__ info,
    u64 *__restrict__ pkey, uint32_t *__restrict__ pent, int32_t *__restrict__ pcopies, uint32_t *__restrict__ pidx,
    typename R::word *__restrict__ tail_out, uint32_t *__restrict__ tsrc, u64 *__restrict__ tlast)
{
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= m || (uint32_t) c >= info[UNIQUE_INFO_CLUSTERS]) return;
    const uint32_t s = start[c], e = start[c + 1];
    const uint32_t first = idx[s], last = idx[e - 1];
    const bool from_tail = first < (uint32_t) n_tail;
    const uint32_t size = e - s - (from_tail ? 1u : 0u);
    const long long t_last = (long long) (tw[last] >> ch_bits) - 1;
    if (from_tail) {
        if (size) atomicAdd(reinterpret_cast<u64 *>(info + UNIQUE_INFO_LATE), (u64) size);
    } else {
        const uint32_t pe = idx[(uint32_t) prim[c]] - (uint32_t) n_tail;    // the primary's ring slot
        const typename R::word *rec = frames + (size_t) pe * R::WORDS;
        const u64 w = tw[pe + (uint32_t) n_tail];
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_PRIMARIES], 1u);
        // the output word: untimed records first by (channel, stamp), then the timed ones by (t, channel)
        pkey[k] = (w >> ch_bits) == 0 ? ((u64) R::channel(rec) << 37) | R::stamp37(rec) : (1ull << 63) | w;
        pent[k] = pe;
        pcopies[k] = (int32_t) size;
        pidx[k] = k;
    }
    if (t_last >= 0 && t_last + window >= rows) {
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_TAIL], 1u);
        if constexpr (R::TAIL_BY_WORDS) {
            tsrc[k] = first;
            tlast[k] = (u64) t_last;
        } else {
            R::store_tail(tail_out + (size_t) k * R::WORDS, R::load(entry_rec<R>(tail, n_tail, frames, first)), t_last);
        }
    }
}

// the next tail where the clusters kernel only noted it: one thread moves one word of an open cluster's first entry
template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_tail_kernel(
    const typename R::word *__restrict__ tail, int n_tail, const typename R::word *__restrict__ frames, int m,
    const uint32_t *__restrict__ info, const uint32_t *__restrict__ tsrc, const u64 *__restrict__ tlast,
    typename R::word *__restrict__ tail_out)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t k = t / R::WORDS, x = t - k * R::WORDS;
    if (k >= (uint32_t) m || k >= info[UNIQUE_INFO_TAIL]) return;
    tail_out[(size_t) k * R::WORDS + x] = R::tail_word(entry_rec<R>(tail, n_tail, frames, tsrc[k])[x], x, tlast[k]);
}

// the primaries in output order: one thread moves one chunk of a record; chunk 0 also its copies and, where the time is
// not in the record, its time
template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_gather_kernel(
    const typename R::word *__restrict__ frames, const long long *__restrict__ times, int np,
    const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent, const int32_t *__restrict__ pcopies,
    typename R::word *__restrict__ out, long long *__restrict__ out_times, int32_t *__restrict__ out_copies)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t q = t / R::CHUNKS, x = t - q * R::CHUNKS;
    if (q >= (uint32_t) np) return;
    const uint32_t k = order[q], e = pent[k];
    reinterpret_cast<typename R::chunk *>(out + (size_t) q * R::WORDS)[x] =
        reinterpret_cast<const typename R::chunk *>(frames + (size_t) e * R::WORDS)[x];
    if (x == 0) {
        if constexpr (!R::TIMED_BY_RECORD) out_times[q] = times[e];
        out_copies[q] = pcopies[k];
    }
}

// ---- the member lists (gnuais_batch_drain_frames_heard, gnuais_batch_drain_long_frames_heard) ----
// ring slot of a primary -> its position in the output; lane 0 also writes first[0] (the scan fills first[1 ..])
__global__ __launch_bounds__(BLOCK) void uniq_slot2q_kernel(
    int np, const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent, uint32_t *__restrict__ slot2q,
    uint32_t *__restrict__ first)
{
    const int q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= np) return;
    slot2q[pent[order[q]]] = (uint32_t) q;
    if (q == 0) first[0] = 0u;
}

// lane = sorted position j: member j - start of its cluster, into the cluster's list.  A cluster behind a tail entry is
// late and listed nowhere.  24 bytes per member at 24 * pos: channel, flags, t and the copy's signal record by ring slot
// (zeros without the array).
template <class R>
__global__ __launch_bounds__(BLOCK) void uniq_heard_kernel(
    int n_tail, const typename R::word *__restrict__ frames, const long long *__restrict__ times,
    const u64 *__restrict__ signal, int m, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ cid,
    const uint32_t *__restrict__ start, const u64 *__restrict__ prim, const uint32_t *__restrict__ slot2q,
    const uint32_t *__restrict__ first, u64 *__restrict__ members)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u, s = start[c];
    if (idx[s] < (uint32_t) n_tail || idx[j] < (uint32_t) n_tail) return;
    const uint32_t e = idx[j] - (uint32_t) n_tail;                          // this member's ring slot
    const uint32_t pe = idx[(uint32_t) prim[c]] - (uint32_t) n_tail;        // the primary's
    const size_t pos = (size_t) first[slot2q[pe]] + ((uint32_t) j - s);
    const typename R::word *rec = frames + (size_t) e * R::WORDS;
    long long t = R::frame_time(rec, times, e);
    if (t < 0) t = -1;
    R::store_hearer(members + 3 * pos, pos, R::channel(rec), R::flags(rec), t, signal ? signal[e] : 0ull);
}

inline dim3 grid_for(size_t n) { return dim3((unsigned) ((n + BLOCK - 1) / BLOCK)); }

template <class R>
hipError_t cluster_enqueue(const UniqueLaunch &a, bool exact, hipStream_t s)
{
    typedef typename R::word word;
    const int m = a.n_tail + a.have;
    if (m <= 0) return hipSuccess;
    if (!a.scratch || a.scratch_bytes < unique_scratch_bytes(m, a.kind) || !a.tail_out ||
        (a.have && (!a.frames || (!R::TIMED_BY_RECORD && !a.times))) || (a.n_tail && !a.tail) || a.window <= 0 ||
        a.hash_bits < 1 || a.hash_bits > 64 || a.ch_bits < 1 || a.ch_bits > 24 || a.time_bits < 1 ||
        a.ch_bits + a.time_bits > 63)
        return hipErrorInvalidValue;
    const Layout l = carve(a.scratch, a.scratch_bytes, (size_t) m, R::TAIL_BY_WORDS);
    const word *tail = static_cast<const word *>(a.tail), *frames = static_cast<const word *>(a.frames);
    const long long *times = reinterpret_cast<const long long *>(a.times);
    const size_t n = (size_t) m;
    size_t t = l.tmp_bytes;
    hipError_t e = hipMemsetAsync(l.info, 0, 4 * UNIQUE_INFO_WORDS, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_keys_kernel<R>, grid_for(n), dim3(BLOCK), 0, s, tail, a.n_tail, frames, times, m, a.ch_bits,
                       a.hash_bits, l.tw, l.hash, l.idxA, l.prim);
    // member order first (stable), then the key: the entries of a key lie together, in (t, channel)
    if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.tw, l.kB, l.idxA, l.idxB, n, 0, a.ch_bits + a.time_bits, s)) != hipSuccess)
        return e;
    uint32_t *cur = l.idxB, *other = l.idxA;
    // the digits of the key, least significant first: the hash alone (pair -1), or the PAIRS pairs of key words
    for (int pair = exact ? R::PAIRS - 1 : -1; pair >= (exact ? 0 : -1); --pair) {
        hipLaunchKernelGGL(uniq_digit_kernel<R>, grid_for(n), dim3(BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.hash,
                           pair, l.kA);
        t = l.tmp_bytes;
        if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, cur, other, n, 0, pair < 0 ? a.hash_bits : 64, s)) != hipSuccess)
            return e;
        std::swap(cur, other);
    }
    hipLaunchKernelGGL(uniq_boundary_kernel<R>, grid_for(n), dim3(BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.kB, l.tw,
                       a.ch_bits, a.window, exact ? 1 : 0, l.head, l.info);
    t = l.tmp_bytes;
    if ((e = rocprim::inclusive_scan(l.tmp, t, l.head, l.cid, n, rocprim::plus<uint32_t>(), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_members_kernel<R>, grid_for(n), dim3(BLOCK), 0, s, a.n_tail, frames, m, cur, l.head, l.cid,
                       l.start, l.prim, l.info);
    // kA / kB are free again: the primaries' output words and their sorted copy
    hipLaunchKernelGGL(uniq_clusters_kernel<R>, grid_for(n), dim3(BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.tw,
                       a.ch_bits, a.window, a.rows, l.start, l.prim, l.info, l.kA, l.pent, l.pcopies, l.pidx,
                       static_cast<word *>(a.tail_out), l.tsrc, l.tlast);
    if constexpr (R::TAIL_BY_WORDS)
        hipLaunchKernelGGL(uniq_tail_kernel<R>, grid_for(n * R::WORDS), dim3(BLOCK), 0, s, tail, a.n_tail, frames, m,
                           l.info, l.tsrc, l.tlast, static_cast<word *>(a.tail_out));
    return hipGetLastError();
}

template <class R>
hipError_t deliver_enqueue(const UniqueLaunch &a, int n_primaries, hipStream_t s)
{
    typedef typename R::word word;
    const int m = a.n_tail + a.have;
    if (n_primaries <= 0) return hipSuccess;
    if (n_primaries > a.have || !a.out_frames || (!R::TIMED_BY_RECORD && !a.out_times) || !a.out_copies)
        return hipErrorInvalidValue;
    const Layout l = carve(a.scratch, a.scratch_bytes, (size_t) m, R::TAIL_BY_WORDS);
    size_t t = l.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, l.pidx, l.pidx2, (size_t) n_primaries, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_gather_kernel<R>, grid_for((size_t) R::CHUNKS * (size_t) n_primaries), dim3(BLOCK), 0, s,
                       static_cast<const word *>(a.frames), reinterpret_cast<const long long *>(a.times), n_primaries,
                       l.pidx2, l.pent, l.pcopies, static_cast<word *>(a.out_frames),
                       reinterpret_cast<long long *>(a.out_times), a.out_copies);
    if (!a.out_first) return hipGetLastError();
    // the member lists: first = the running sum of the copies in output order; then every member of a delivered
    // cluster finds its cluster's list through the primary's ring slot
    if (!a.out_members || (reinterpret_cast<uintptr_t>(a.out_members) & (uintptr_t) (R::MEMBER_ALIGN - 1)) ||
        !a.heard_scratch || a.heard_scratch_bytes < unique_heard_scratch_bytes(a.have))
        return hipErrorInvalidValue;
    uint32_t *slot2q = static_cast<uint32_t *>(a.heard_scratch), *first = reinterpret_cast<uint32_t *>(a.out_first);
    t = l.tmp_bytes;
    e = rocprim::inclusive_scan(l.tmp, t, reinterpret_cast<const uint32_t *>(a.out_copies), first + 1, (size_t) n_primaries,
                                rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_slot2q_kernel, grid_for((size_t) n_primaries), dim3(BLOCK), 0, s, n_primaries, l.pidx2, l.pent,
                       slot2q, first);
    // the sorted index array is idxA in both attempts: one sort into idxB, then one (hashed) or PAIRS (exact, odd) more
    hipLaunchKernelGGL(uniq_heard_kernel<R>, grid_for((size_t) m), dim3(BLOCK), 0, s, a.n_tail,
                       static_cast<const word *>(a.frames), reinterpret_cast<const long long *>(a.times),
                       static_cast<const u64 *>(a.signal), m, l.idxA, l.cid, l.start, l.prim, slot2q, first,
                       reinterpret_cast<u64 *>(a.out_members));
    return hipGetLastError();
}

} // namespace

size_t unique_heard_scratch_bytes(int have) { return slot(4 * (size_t) (have > 0 ? have : 1)); }

size_t unique_scratch_bytes(int n_entries, UniqueKind kind)
{
    const size_t m = (size_t) (n_entries > 0 ? n_entries : 1), by_words = kind == UniqueKind::Long ? 1 : 0;
    return slot(4 * UNIQUE_INFO_WORDS) + (5 + by_words) * slot(8 * m) + (8 + by_words) * slot(4 * m) + slot(4 * (m + 1)) +
           rocprim_tmp_bytes(m) + 256;
}

uint32_t *unique_info(void *scratch) { return static_cast<uint32_t *>(scratch); }

hipError_t unique_cluster_enqueue(const UniqueLaunch &a, bool exact, hipStream_t s)
{
    return a.kind == UniqueKind::Long ? cluster_enqueue<LongDev>(a, exact, s) : cluster_enqueue<ShortDev>(a, exact, s);
}

hipError_t unique_deliver_enqueue(const UniqueLaunch &a, int n_primaries, hipStream_t s)
{
    return a.kind == UniqueKind::Long ? deliver_enqueue<LongDev>(a, n_primaries, s) : deliver_enqueue<ShortDev>(a, n_primaries, s);
}

} // namespace gnuais
