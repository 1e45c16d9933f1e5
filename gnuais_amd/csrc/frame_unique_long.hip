// frame_unique_long.hip -- the duplicate merge of the long frames on the device (definition: include/gnuais_hip.h,
// gnuais_batch_long_unique; the host statement it must equal bit for bit: frame_unique.cpp over LongRec).
//
// The pipeline is frame_unique.hip's, stage by stage, over records of another shape (frame_unique.h: LongRec).  A
// gnuais_long_frame is 152 bytes and 8-byte aligned only, so every record access here is in 64-bit words, 19 per record:
// word 0 channel | end_bit << 32, word 1 t, word 2 nbits | flags << 16 | reserved << 24 | payload[0..3] << 32, words 3..18
// the rest of the payload.  The key is words 2..18 with word 2 masked (LongRec::KEY_FIRST_MASK64): 17 words, the 17 pairs
// of the definition.  The member time is the record's own word 1; there is no times array.
// Entries are [tail | long ring]; a tail entry is a record with t_last in word 1 and word 2 masked to the key.
// Nothing runs per call: the whole stage is the drain.  No LDS, no scratch memory.
//
//   keys      lane = entry: the member-order word (t + 1) << ch_bits | channel and a 64-bit hash of the 17 key words
//   sort      stable radix sort by the order word, then by the hash: every key's entries lie together in member order
//   digit     lane = sorted position: the hash, or one key word, of the entry there: the next stable sort's digit
//   boundary  lane = position: is the neighbour before it the same key (hash AND the 17 words; the second record is
//             read only where the hashes are equal) and within the window?  Equal hashes with unequal keys raise the
//             collision flag: the caller repeats the sort in its exact form -- 17 stable sorts by the key words in place
//             of the one by the hash
//   scan      cluster number of every position
//   members   lane = position: the cluster's start, and an atomic minimum of (repaired, position) -- the primary
//   clusters  lane = cluster: copies, late copies, the primary into a compacted list with its output word; a cluster that
//             stays open gets a slot of the next tail: its first entry and t_last are noted
//   tail      thread = (tail slot, 64-bit word): the noted entry's record into the next tail, adjacent lanes on adjacent
//             words; word 1 is t_last, word 2 is masked
//   deliver   sort of the primaries by the output word; gather with thread = (record, 64-bit word): 156 bytes per
//             delivered record cross PCIe
//   heard     only where the member lists are wanted: the scan of the copies, the map from a primary's ring slot to its
//             output position, and per sorted position the member's 24 bytes (three 64-bit stores)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "frame_unique.h"
#include "kernels.h"

namespace gnuais {

namespace {

typedef uniq::LongRec LR;
constexpr int LQ_BLOCK = 256;
constexpr int W64 = LR::REC_WORDS64;            // 19
typedef unsigned long long u64;

// the scratch of one drain of m entries, 256-byte slots
struct LongLayout {
    uint32_t *info;             // UNIQUE_INFO_WORDS
    u64 *tw, *hash, *kA, *kB, *prim, *tlast;
    uint32_t *idxA, *idxB, *head, *cid, *start, *pent, *pidx, *pidx2, *tsrc;
    int32_t *pcopies;
    void *tmp;
    size_t tmp_bytes;
};

size_t long_rocprim_tmp_bytes(size_t m)
{
    size_t sort_tmp = 0, scan_tmp = 0;
    (void) rocprim::radix_sort_pairs(nullptr, sort_tmp, (u64 *) nullptr, (u64 *) nullptr, (uint32_t *) nullptr,
                                     (uint32_t *) nullptr, m, 0, 64, (hipStream_t) 0);
    (void) rocprim::inclusive_scan(nullptr, scan_tmp, (uint32_t *) nullptr, (uint32_t *) nullptr, m,
                                   rocprim::plus<uint32_t>(), (hipStream_t) 0);
    return sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
}

inline size_t lslot(size_t bytes) { return (bytes + 255) / 256 * 256; }

LongLayout long_carve(void *scratch, size_t scratch_bytes, size_t m)
{
    char *p = static_cast<char *>(scratch);
    auto take = [&](size_t bytes) { char *q = p; p += lslot(bytes); return (void *) q; };
    LongLayout l;
    l.info = (uint32_t *) take(4 * UNIQUE_INFO_WORDS);
    l.tw = (u64 *) take(8 * m);
    l.hash = (u64 *) take(8 * m);
    l.kA = (u64 *) take(8 * m);
    l.kB = (u64 *) take(8 * m);
    l.prim = (u64 *) take(8 * m);
    l.tlast = (u64 *) take(8 * m);
    l.idxA = (uint32_t *) take(4 * m);
    l.idxB = (uint32_t *) take(4 * m);
    l.head = (uint32_t *) take(4 * m);
    l.cid = (uint32_t *) take(4 * m);
    l.start = (uint32_t *) take(4 * (m + 1));
    l.pent = (uint32_t *) take(4 * m);
    l.pidx = (uint32_t *) take(4 * m);
    l.pidx2 = (uint32_t *) take(4 * m);
    l.tsrc = (uint32_t *) take(4 * m);
    l.pcopies = (int32_t *) take(4 * m);
    l.tmp = p;
    l.tmp_bytes = scratch_bytes - (size_t) (p - static_cast<char *>(scratch));
    return l;
}

// entry i of [tail | ring]: its 19 words
__device__ __forceinline__ const u64 *entry64(const u64 *tail, int n_tail, const u64 *frames, uint32_t i)
{
    return i < (uint32_t) n_tail ? tail + (size_t) i * W64 : frames + (size_t) (i - (uint32_t) n_tail) * W64;
}

__global__ __launch_bounds__(LQ_BLOCK) void luniq_keys_kernel(
    const u64 *__restrict__ tail, int n_tail, const u64 *__restrict__ frames, int m, int ch_bits, int hash_bits,
    u64 *__restrict__ tw, u64 *__restrict__ hash, uint32_t *__restrict__ idx, u64 *__restrict__ prim)
{
    const int i = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 *q = entry64(tail, n_tail, frames, (uint32_t) i);
    long long t = (long long) q[LR::T_WORD64];
    uint32_t ch = 0;
    if (i >= n_tail) {
        if (t < -1) t = -1;
        ch = (uint32_t) q[0];
    }
    u64 h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int p = 0; p < LR::KEY_PAIRS; ++p) {
        h ^= LR::key_word64(q[LR::KEY_WORD64 + p], p);
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
__global__ __launch_bounds__(LQ_BLOCK) void luniq_digit_kernel(
    const u64 *__restrict__ tail, int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ idx,
    const u64 *__restrict__ hash, int pair, u64 *__restrict__ out)
{
    const int j = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t e = idx[j];
    out[j] = pair < 0 ? hash[e] : LR::key_word64(entry64(tail, n_tail, frames, e)[LR::KEY_WORD64 + pair], pair);
}

__global__ __launch_bounds__(LQ_BLOCK) void luniq_boundary_kernel(
    const u64 *__restrict__ tail, int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ idx,
    const u64 *__restrict__ hs, const u64 *__restrict__ tw, int ch_bits, long long window, int exact,
    uint32_t *__restrict__ head, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    uint32_t is_head = 1;
    if (j > 0 && (exact || hs[j] == hs[j - 1])) {
        const uint32_t e = idx[j], p = idx[j - 1];
        const u64 *a = entry64(tail, n_tail, frames, e), *b = entry64(tail, n_tail, frames, p);
        u64 diff = 0;
#pragma unroll
        for (int k = 0; k < LR::KEY_PAIRS; ++k) diff |= LR::key_word64(a[LR::KEY_WORD64 + k] ^ b[LR::KEY_WORD64 + k], k);
        if (diff) {
            if (!exact) info[UNIQUE_INFO_COLLISION] = 1u;      // every writer writes the same word
        } else {
            const long long te = (long long) (tw[e] >> ch_bits) - 1, tp = (long long) (tw[p] >> ch_bits) - 1;
            if (te >= 0 && tp >= 0 && te - tp <= window) is_head = 0;
        }
    }
    head[j] = is_head;
}

__global__ __launch_bounds__(LQ_BLOCK) void luniq_members_kernel(
    int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ cid, uint32_t *__restrict__ start, u64 *__restrict__ prim, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u;             // cid is an inclusive sum that starts with a head: >= 1
    if (head[j]) start[c] = (uint32_t) j;
    if (j == m - 1) {
        start[c + 1] = (uint32_t) m;
        info[UNIQUE_INFO_CLUSTERS] = c + 1u;
    }
    const uint32_t e = idx[j];
    if (e >= (uint32_t) n_tail) {
        const u64 q2 = frames[(size_t) (e - (uint32_t) n_tail) * W64 + LR::KEY_WORD64];
        atomicMin(&prim[c], ((u64) LR::repaired_bit64(q2) << 32) | (u64) (uint32_t) j);
    }
}

__global__ __launch_bounds__(LQ_BLOCK) void luniq_clusters_kernel(
    int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ idx, const u64 *__restrict__ tw,
    int ch_bits, long long window, long long rows, const uint32_t *__restrict__ start, const u64 *__restrict__ prim,
    uint32_t *__restrict__ info, u64 *__restrict__ pkey, uint32_t *__restrict__ pent, int32_t *__restrict__ pcopies,
    uint32_t *__restrict__ pidx, uint32_t *__restrict__ tsrc, u64 *__restrict__ tlast)
{
    const int c = blockIdx.x * LQ_BLOCK + threadIdx.x;
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
        const u64 *rec = frames + (size_t) pe * W64;
        const u64 w = tw[pe + (uint32_t) n_tail];
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_PRIMARIES], 1u);
        // the output word: untimed records first by (channel, stamp), then the timed ones by (t, channel)
        pkey[k] = (w >> ch_bits) == 0 ? ((rec[0] & 0xffffffffull) << 37) | LR::stamp37_64(rec[0], rec[LR::KEY_WORD64])
                                      : (1ull << 63) | w;
        pent[k] = pe;
        pcopies[k] = (int32_t) size;
        pidx[k] = k;
    }
    if (t_last >= 0 && t_last + window >= rows) {
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_TAIL], 1u);
        tsrc[k] = first;
        tlast[k] = (u64) t_last;
    }
}

// the next tail: one thread moves one 64-bit word of an open cluster's first entry; word 1 is t_last, word 2 the masked key
__global__ __launch_bounds__(LQ_BLOCK) void luniq_tail_kernel(
    const u64 *__restrict__ tail, int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ info,
    const uint32_t *__restrict__ tsrc, const u64 *__restrict__ tlast, u64 *__restrict__ tail_out)
{
    const uint32_t t = blockIdx.x * LQ_BLOCK + threadIdx.x;
    const uint32_t k = t / W64, x = t - k * W64;
    if (k >= (uint32_t) m || k >= info[UNIQUE_INFO_TAIL]) return;
    u64 v = entry64(tail, n_tail, frames, tsrc[k])[x];
    if (x == LR::T_WORD64) v = tlast[k];
    if (x == LR::KEY_WORD64) v &= LR::KEY_FIRST_MASK64;
    tail_out[(size_t) k * W64 + x] = v;
}

// the primaries in output order: one thread moves one 64-bit word of a record; word 0 also its copies
__global__ __launch_bounds__(LQ_BLOCK) void luniq_gather_kernel(
    const u64 *__restrict__ frames, int np, const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent,
    const int32_t *__restrict__ pcopies, u64 *__restrict__ out, int32_t *__restrict__ out_copies)
{
    const uint32_t t = blockIdx.x * LQ_BLOCK + threadIdx.x;
    const uint32_t q = t / W64, x = t - q * W64;
    if (q >= (uint32_t) np) return;
    const uint32_t k = order[q], e = pent[k];
    out[(size_t) q * W64 + x] = frames[(size_t) e * W64 + x];
    if (x == 0) out_copies[q] = pcopies[k];
}

// ---- the member lists (gnuais_batch_drain_long_frames_heard) ----
// ring slot of a primary -> its position in the output; lane 0 also writes first[0] (the scan fills first[1 ..])
__global__ __launch_bounds__(LQ_BLOCK) void luniq_slot2q_kernel(
    int np, const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent, uint32_t *__restrict__ slot2q,
    uint32_t *__restrict__ first)
{
    const int q = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (q >= np) return;
    slot2q[pent[order[q]]] = (uint32_t) q;
    if (q == 0) first[0] = 0u;
}

// lane = sorted position j: member j - start of its cluster, into the cluster's list.  A cluster behind a tail entry is
// late and listed nowhere.  24 bytes per member: channel | flags << 32, t, and the copy's signal record by ring slot
// (long_signal.hip; zeros without the array).
__global__ __launch_bounds__(LQ_BLOCK) void luniq_heard_kernel(
    int n_tail, const u64 *__restrict__ frames, int m, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ cid,
    const uint32_t *__restrict__ start, const u64 *__restrict__ prim, const uint32_t *__restrict__ slot2q,
    const uint32_t *__restrict__ first, const u64 *__restrict__ signal, u64 *__restrict__ members)
{
    const int j = blockIdx.x * LQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u, s = start[c];
    if (idx[s] < (uint32_t) n_tail || idx[j] < (uint32_t) n_tail) return;
    const uint32_t e = idx[j] - (uint32_t) n_tail;                          // this member's ring slot
    const uint32_t pe = idx[(uint32_t) prim[c]] - (uint32_t) n_tail;        // the primary's
    const size_t pos = (size_t) first[slot2q[pe]] + ((uint32_t) j - s);
    const u64 *rec = frames + (size_t) e * W64;
    long long t = (long long) rec[LR::T_WORD64];
    if (t < 0) t = -1;
    u64 *out = members + 3 * pos;
    out[0] = (rec[0] & 0xffffffffull) | ((u64) LR::flags64(rec[LR::KEY_WORD64]) << 32);
    out[1] = (u64) t;
    out[2] = signal ? signal[e] : 0ull;
}

inline dim3 lgrid_for(size_t n) { return dim3((unsigned) ((n + LQ_BLOCK - 1) / LQ_BLOCK)); }

} // namespace

size_t long_unique_heard_scratch_bytes(int have) { return lslot(4 * (size_t) (have > 0 ? have : 1)); }

size_t long_unique_scratch_bytes(int n_entries)
{
    const size_t m = (size_t) (n_entries > 0 ? n_entries : 1);
    return lslot(4 * UNIQUE_INFO_WORDS) + 6 * lslot(8 * m) + 9 * lslot(4 * m) + lslot(4 * (m + 1)) + long_rocprim_tmp_bytes(m) + 256;
}

uint32_t *long_unique_info(void *scratch) { return static_cast<uint32_t *>(scratch); }

hipError_t long_unique_cluster_enqueue(const LongUniqueLaunch &a, bool exact, hipStream_t s)
{
    const int m = a.n_tail + a.have;
    if (m <= 0) return hipSuccess;
    if (!a.scratch || a.scratch_bytes < long_unique_scratch_bytes(m) || !a.tail_out || (a.have && !a.frames) ||
        (a.n_tail && !a.tail) || a.window <= 0 || a.hash_bits < 1 || a.hash_bits > 64 || a.ch_bits < 1 || a.ch_bits > 24 ||
        a.time_bits < 1 || a.ch_bits + a.time_bits > 63)
        return hipErrorInvalidValue;
    const LongLayout l = long_carve(a.scratch, a.scratch_bytes, (size_t) m);
    const u64 *tail = static_cast<const u64 *>(a.tail), *frames = static_cast<const u64 *>(a.frames);
    const size_t n = (size_t) m;
    size_t t = l.tmp_bytes;
    hipError_t e = hipMemsetAsync(l.info, 0, 4 * UNIQUE_INFO_WORDS, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(luniq_keys_kernel, lgrid_for(n), dim3(LQ_BLOCK), 0, s, tail, a.n_tail, frames, m, a.ch_bits,
                       a.hash_bits, l.tw, l.hash, l.idxA, l.prim);
    // member order first (stable), then the key: the entries of a key lie together, in (t, channel)
    if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.tw, l.kB, l.idxA, l.idxB, n, 0, a.ch_bits + a.time_bits, s)) != hipSuccess)
        return e;
    uint32_t *cur = l.idxB, *other = l.idxA;
    // the digits of the key, least significant first: the hash alone (pair -1), or the 17 pairs of key words
    for (int pair = exact ? LR::KEY_PAIRS - 1 : -1; pair >= (exact ? 0 : -1); --pair) {
        hipLaunchKernelGGL(luniq_digit_kernel, lgrid_for(n), dim3(LQ_BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.hash,
                           pair, l.kA);
        t = l.tmp_bytes;
        if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, cur, other, n, 0, pair < 0 ? a.hash_bits : 64, s)) != hipSuccess)
            return e;
        std::swap(cur, other);
    }
    hipLaunchKernelGGL(luniq_boundary_kernel, lgrid_for(n), dim3(LQ_BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.kB,
                       l.tw, a.ch_bits, a.window, exact ? 1 : 0, l.head, l.info);
    t = l.tmp_bytes;
    if ((e = rocprim::inclusive_scan(l.tmp, t, l.head, l.cid, n, rocprim::plus<uint32_t>(), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(luniq_members_kernel, lgrid_for(n), dim3(LQ_BLOCK), 0, s, a.n_tail, frames, m, cur, l.head, l.cid,
                       l.start, l.prim, l.info);
    // kA / kB are free again: the primaries' output words and their sorted copy
    hipLaunchKernelGGL(luniq_clusters_kernel, lgrid_for(n), dim3(LQ_BLOCK), 0, s, a.n_tail, frames, m, cur, l.tw, a.ch_bits,
                       a.window, a.rows, l.start, l.prim, l.info, l.kA, l.pent, l.pcopies, l.pidx, l.tsrc, l.tlast);
    hipLaunchKernelGGL(luniq_tail_kernel, lgrid_for(n * W64), dim3(LQ_BLOCK), 0, s, tail, a.n_tail, frames, m, l.info, l.tsrc,
                       l.tlast, static_cast<u64 *>(a.tail_out));
    return hipGetLastError();
}

hipError_t long_unique_deliver_enqueue(const LongUniqueLaunch &a, int n_primaries, hipStream_t s)
{
    const int m = a.n_tail + a.have;
    if (n_primaries <= 0) return hipSuccess;
    if (n_primaries > a.have || !a.out_frames || !a.out_copies) return hipErrorInvalidValue;
    const LongLayout l = long_carve(a.scratch, a.scratch_bytes, (size_t) m);
    size_t t = l.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, l.pidx, l.pidx2, (size_t) n_primaries, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(luniq_gather_kernel, lgrid_for((size_t) W64 * (size_t) n_primaries), dim3(LQ_BLOCK), 0, s,
                       static_cast<const u64 *>(a.frames), n_primaries, l.pidx2, l.pent, l.pcopies,
                       reinterpret_cast<u64 *>(a.out_frames), a.out_copies);
    if (!a.out_first) return hipGetLastError();
    // the member lists: first = the running sum of the copies in output order; then every member of a delivered
    // cluster finds its cluster's list through the primary's ring slot
    if (!a.out_members || (reinterpret_cast<uintptr_t>(a.out_members) & 7u) || !a.heard_scratch ||
        a.heard_scratch_bytes < long_unique_heard_scratch_bytes(a.have))
        return hipErrorInvalidValue;
    uint32_t *slot2q = static_cast<uint32_t *>(a.heard_scratch), *first = reinterpret_cast<uint32_t *>(a.out_first);
    t = l.tmp_bytes;
    e = rocprim::inclusive_scan(l.tmp, t, reinterpret_cast<const uint32_t *>(a.out_copies), first + 1, (size_t) n_primaries,
                                rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(luniq_slot2q_kernel, lgrid_for((size_t) n_primaries), dim3(LQ_BLOCK), 0, s, n_primaries, l.pidx2,
                       l.pent, slot2q, first);
    // the sorted index array is idxA in both attempts: one sort into idxB, then one (hashed) or 17 (exact) more
    hipLaunchKernelGGL(luniq_heard_kernel, lgrid_for((size_t) m), dim3(LQ_BLOCK), 0, s, a.n_tail,
                       static_cast<const u64 *>(a.frames), m, l.idxA, l.cid, l.start, l.prim, slot2q, first,
                       static_cast<const u64 *>(a.signal), reinterpret_cast<u64 *>(a.out_members));
    return hipGetLastError();
}

} // namespace gnuais
