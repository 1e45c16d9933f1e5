// frame_unique.hip -- the duplicate merge on the device (definition: include/gnuais_hip.h, gnuais_batch_unique; the
// host statement it must equal bit for bit: frame_unique.cpp).
//
// Nothing runs per call: the whole stage is the drain.  Entries are [tail | ring]: the open clusters an earlier drain
// left behind (16 words each: t_last in words 0..1, the key in words 2..15 as in a record) and the frames K3 appended,
// with their times.  Lane = entry (or sorted position, or cluster) in every kernel; no LDS, no scratch memory.
//
//   keys      per entry: the member-order word (t + 1) << ch_bits | channel and a 64-bit hash of the 14 key words
//   sort      stable radix sort by the order word, then by the hash: every key's entries lie together in member order
//   boundary  per position: is the neighbour before it the same key (hash AND the 14 words) and within the window?
//             Equal hashes with unequal keys raise the collision flag: the caller then repeats the sort in its exact
//             form -- seven stable sorts by the key words themselves in place of the one by the hash -- so the result
//             never depends on the hash (set_option("unique_hash_bits") truncates it for the tests).
//   scan      cluster number of every position (inclusive sum of the head flags)
//   members   per position: the cluster's start, and an atomic minimum of (repaired, position) over its frames -- the
//             primary; a minimum does not depend on arrival order, and a cluster may be any size
//   clusters  per cluster: copies, late copies (behind a tail entry), the primary into a compacted list with its output
//             order word, the cluster into the next tail if its last member is within the window of `rows`
//   deliver   sort of the primaries by the output word (unique per record, so the slot order of the compaction does
//             not show), gather of records, times and copies: 76 bytes per delivered frame cross PCIe
//   heard     only where the member lists are wanted (gnuais_batch_drain_frames_heard): scan of the copies in output
//             order = the lists' offsets, a map from a primary's ring slot to its output position, and per sorted
//             position the member's 24 bytes into its cluster's list (a cluster's members lie together in the sort)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "frame_unique.h"
#include "kernels.h"

namespace gnuais {

using namespace uniq;

namespace {

constexpr int UQ_BLOCK = 256;
typedef unsigned long long u64;

// the scratch of one drain of m entries, 256-byte slots
struct Layout {
    uint32_t *info;             // UNIQUE_INFO_WORDS
    u64 *tw, *hash, *kA, *kB, *prim;
    uint32_t *idxA, *idxB, *head, *cid, *start, *pent, *pidx, *pidx2;
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

Layout carve(void *scratch, size_t scratch_bytes, size_t m)
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
    l.idxA = (uint32_t *) take(4 * m);
    l.idxB = (uint32_t *) take(4 * m);
    l.head = (uint32_t *) take(4 * m);
    l.cid = (uint32_t *) take(4 * m);
    l.start = (uint32_t *) take(4 * (m + 1));
    l.pent = (uint32_t *) take(4 * m);
    l.pidx = (uint32_t *) take(4 * m);
    l.pidx2 = (uint32_t *) take(4 * m);
    l.pcopies = (int32_t *) take(4 * m);
    l.tmp = p;
    l.tmp_bytes = scratch_bytes - (size_t) (p - static_cast<char *>(scratch));
    return l;
}

// entry i of [tail | ring]: its 16 words
__device__ __forceinline__ const uint32_t *entry_rec(const uint32_t *tail, int n_tail, const uint32_t *frames, uint32_t i)
{
    return i < (uint32_t) n_tail ? tail + (size_t) i * 16 : frames + (size_t) (i - (uint32_t) n_tail) * 16;
}

__device__ __forceinline__ void load_rec(const uint32_t *rec, uint32_t w[16])
{
    const uint4 *q = reinterpret_cast<const uint4 *>(rec);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 v = q[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
}

__global__ __launch_bounds__(UQ_BLOCK) void uniq_keys_kernel(
    const uint32_t *__restrict__ tail, int n_tail, const uint32_t *__restrict__ frames,
    const long long *__restrict__ times, int m, int ch_bits, int hash_bits, u64 *__restrict__ tw,
    u64 *__restrict__ hash, uint32_t *__restrict__ idx, u64 *__restrict__ prim)
{
    const int i = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t w[16];
    load_rec(entry_rec(tail, n_tail, frames, (uint32_t) i), w);
    long long t;
    uint32_t ch = 0;
    if (i < n_tail) {
        t = (long long) ((u64) w[0] | ((u64) w[1] << 32));
    } else {
        t = times[i - n_tail];
        if (t < -1) t = -1;
        ch = w[0];
    }
    u64 h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int k = 0; k < KEY_WORDS; k += 2) {
        const u64 x = (u64) key_word(w, k) | ((u64) key_word(w, k + 1) << 32);
        h ^= x;
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
__global__ __launch_bounds__(UQ_BLOCK) void uniq_digit_kernel(
    const uint32_t *__restrict__ tail, int n_tail, const uint32_t *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ hash, int pair, u64 *__restrict__ out)
{
    const int j = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t e = idx[j];
    if (pair < 0) {
        out[j] = hash[e];
        return;
    }
    const uint32_t *rec = entry_rec(tail, n_tail, frames, e);
    const uint32_t hi = pair == 6 ? rec[14] : rec[2 + 2 * pair];
    const uint32_t lo = pair == 6 ? rec[15] & KEY_LAST_MASK : rec[3 + 2 * pair];
    out[j] = ((u64) hi << 32) | lo;
}

__global__ __launch_bounds__(UQ_BLOCK) void uniq_boundary_kernel(
    const uint32_t *__restrict__ tail, int n_tail, const uint32_t *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ hs, const u64 *__restrict__ tw, int ch_bits,
    long long window, int exact, uint32_t *__restrict__ head, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    uint32_t is_head = 1;
    if (j > 0 && (exact || hs[j] == hs[j - 1])) {
        const uint32_t e = idx[j], p = idx[j - 1];
        uint32_t a[16], b[16];
        load_rec(entry_rec(tail, n_tail, frames, e), a);
        load_rec(entry_rec(tail, n_tail, frames, p), b);
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < KEY_WORDS; ++k) diff |= key_word(a, k) ^ key_word(b, k);
        if (diff) {
            if (!exact) info[UNIQUE_INFO_COLLISION] = 1u;      // every writer writes the same word
        } else {
            const long long te = (long long) (tw[e] >> ch_bits) - 1, tp = (long long) (tw[p] >> ch_bits) - 1;
            if (te >= 0 && tp >= 0 && te - tp <= window) is_head = 0;
        }
    }
    head[j] = is_head;
}

__global__ __launch_bounds__(UQ_BLOCK) void uniq_members_kernel(
    int n_tail, const uint32_t *__restrict__ frames, int m, const uint32_t *__restrict__ idx,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ cid, uint32_t *__restrict__ start,
    u64 *__restrict__ prim, uint32_t *__restrict__ info)
{
    const int j = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u;             // cid is an inclusive sum that starts with a head: >= 1
    if (head[j]) start[c] = (uint32_t) j;
    if (j == m - 1) {
        start[c + 1] = (uint32_t) m;
        info[UNIQUE_INFO_CLUSTERS] = c + 1u;
    }
    const uint32_t e = idx[j];
    if (e >= (uint32_t) n_tail) {
        const uint32_t *rec = frames + (size_t) (e - (uint32_t) n_tail) * 16;
        atomicMin(&prim[c], ((u64) repaired_bit(rec) << 32) | (u64) (uint32_t) j);
    }
}

__global__ __launch_bounds__(UQ_BLOCK) void uniq_clusters_kernel(
    const uint32_t *__restrict__ tail, int n_tail, const uint32_t *__restrict__ frames, int m,
    const uint32_t *__restrict__ idx, const u64 *__restrict__ tw, int ch_bits, long long window, long long rows,
    const uint32_t *__restrict__ start, const u64 *__restrict__ prim, uint32_t *__restrict__ info,
    u64 *__restrict__ pkey, uint32_t *__restrict__ pent, int32_t *__restrict__ pcopies, uint32_t *__restrict__ pidx,
    uint32_t *__restrict__ tail_out)
{
    const int c = blockIdx.x * UQ_BLOCK + threadIdx.x;
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
        const uint32_t *rec = frames + (size_t) pe * 16;
        const u64 w = tw[pe + (uint32_t) n_tail];
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_PRIMARIES], 1u);
        // the output word: untimed records first by (channel, stamp), then the timed ones by (t, channel)
        pkey[k] = (w >> ch_bits) == 0 ? ((u64) rec[0] << 37) | stamp37(rec) : (1ull << 63) | w;
        pent[k] = pe;
        pcopies[k] = (int32_t) size;
        pidx[k] = k;
    }
    if (t_last >= 0 && t_last + window >= rows) {
        const uint32_t k = atomicAdd(&info[UNIQUE_INFO_TAIL], 1u);
        uint32_t w[16];
        load_rec(entry_rec(tail, n_tail, frames, first), w);
        w[0] = (uint32_t) ((u64) t_last & 0xffffffffull);
        w[1] = (uint32_t) ((u64) t_last >> 32);
        w[15] &= KEY_LAST_MASK;
        uint4 *q = reinterpret_cast<uint4 *>(tail_out + (size_t) k * 16);
#pragma unroll
        for (int x = 0; x < 4; ++x) q[x] = make_uint4(w[4 * x], w[4 * x + 1], w[4 * x + 2], w[4 * x + 3]);
    }
}

// the primaries in output order: one thread moves one 16-byte quarter of a record; quarter 0 also its time and copies
__global__ __launch_bounds__(UQ_BLOCK) void uniq_gather_kernel(
    const uint32_t *__restrict__ frames, const long long *__restrict__ times, int np,
    const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent, const int32_t *__restrict__ pcopies,
    uint32_t *__restrict__ out, long long *__restrict__ out_times, int32_t *__restrict__ out_copies)
{
    const int t = blockIdx.x * UQ_BLOCK + threadIdx.x;
    const int q = t >> 2, x = t & 3;
    if (q >= np) return;
    const uint32_t k = order[q], e = pent[k];
    reinterpret_cast<uint4 *>(out + (size_t) q * 16)[x] = reinterpret_cast<const uint4 *>(frames + (size_t) e * 16)[x];
    if (x == 0) {
        out_times[q] = times[e];
        out_copies[q] = pcopies[k];
    }
}

// ---- the member lists (gnuais_batch_drain_frames_heard) ----
// ring slot of a primary -> its position in the output; lane 0 also writes first[0] (the scan fills first[1 ..])
__global__ __launch_bounds__(UQ_BLOCK) void uniq_slot2q_kernel(
    int np, const uint32_t *__restrict__ order, const uint32_t *__restrict__ pent, uint32_t *__restrict__ slot2q,
    uint32_t *__restrict__ first)
{
    const int q = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (q >= np) return;
    slot2q[pent[order[q]]] = (uint32_t) q;
    if (q == 0) first[0] = 0u;
}

// lane = sorted position j: member j - start of its cluster, into the cluster's list.  A cluster behind a tail entry is
// late and listed nowhere.  24 bytes per member at 24 * pos: the 16-byte store takes whichever half is 16-aligned.
__global__ __launch_bounds__(UQ_BLOCK) void uniq_heard_kernel(
    int n_tail, const uint32_t *__restrict__ frames, const long long *__restrict__ times,
    const u64 *__restrict__ signal, int m, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ cid,
    const uint32_t *__restrict__ start, const u64 *__restrict__ prim, const uint32_t *__restrict__ slot2q,
    const uint32_t *__restrict__ first, u64 *__restrict__ members)
{
    const int j = blockIdx.x * UQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cid[j] - 1u, s = start[c];
    if (idx[s] < (uint32_t) n_tail || idx[j] < (uint32_t) n_tail) return;
    const uint32_t e = idx[j] - (uint32_t) n_tail;                          // this member's ring slot
    const uint32_t pe = idx[(uint32_t) prim[c]] - (uint32_t) n_tail;        // the primary's
    const size_t pos = (size_t) first[slot2q[pe]] + ((uint32_t) j - s);
    const uint32_t *rec = frames + (size_t) e * 16;
    const uint32_t channel = rec[0], flags = (rec[15] >> 8) & 0xffu;
    long long t = times[e];
    if (t < 0) t = -1;
    const u64 sig = signal ? signal[e] : 0ull;
    const uint32_t t_lo = (uint32_t) ((u64) t & 0xffffffffull), t_hi = (uint32_t) ((u64) t >> 32);
    u64 *out = members + 3 * pos;
    if ((pos & 1) == 0) {
        *reinterpret_cast<uint4 *>(out) = make_uint4(channel, flags, t_lo, t_hi);
        out[2] = sig;
    } else {
        out[0] = (u64) channel | ((u64) flags << 32);
        *reinterpret_cast<uint4 *>(out + 1) = make_uint4(t_lo, t_hi, (uint32_t) (sig & 0xffffffffull), (uint32_t) (sig >> 32));
    }
}

inline dim3 grid_for(size_t n) { return dim3((unsigned) ((n + UQ_BLOCK - 1) / UQ_BLOCK)); }

} // namespace

size_t unique_heard_scratch_bytes(int have) { return slot(4 * (size_t) (have > 0 ? have : 1)); }

size_t unique_scratch_bytes(int n_entries)
{
    const size_t m = (size_t) (n_entries > 0 ? n_entries : 1);
    return slot(4 * UNIQUE_INFO_WORDS) + 5 * slot(8 * m) + 8 * slot(4 * m) + slot(4 * (m + 1)) + rocprim_tmp_bytes(m) + 256;
}

uint32_t *unique_info(void *scratch) { return static_cast<uint32_t *>(scratch); }

hipError_t unique_cluster_enqueue(const UniqueLaunch &a, bool exact, hipStream_t s)
{
    const int m = a.n_tail + a.have;
    if (m <= 0) return hipSuccess;
    if (!a.scratch || a.scratch_bytes < unique_scratch_bytes(m) || !a.tail_out || (a.have && (!a.frames || !a.times)) ||
        (a.n_tail && !a.tail) || a.window <= 0 || a.hash_bits < 1 || a.hash_bits > 64 || a.ch_bits < 1 || a.ch_bits > 24 ||
        a.time_bits < 1 || a.ch_bits + a.time_bits > 63)
        return hipErrorInvalidValue;
    const Layout l = carve(a.scratch, a.scratch_bytes, (size_t) m);
    const uint32_t *tail = static_cast<const uint32_t *>(a.tail), *frames = static_cast<const uint32_t *>(a.frames);
    const long long *times = reinterpret_cast<const long long *>(a.times);
    const size_t n = (size_t) m;
    size_t t = l.tmp_bytes;
    hipError_t e = hipMemsetAsync(l.info, 0, 4 * UNIQUE_INFO_WORDS, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_keys_kernel, grid_for(n), dim3(UQ_BLOCK), 0, s, tail, a.n_tail, frames, times, m, a.ch_bits,
                       a.hash_bits, l.tw, l.hash, l.idxA, l.prim);
    // member order first (stable), then the key: the entries of a key lie together, in (t, channel)
    if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.tw, l.kB, l.idxA, l.idxB, n, 0, a.ch_bits + a.time_bits, s)) != hipSuccess)
        return e;
    uint32_t *cur = l.idxB, *other = l.idxA;
    // the digits of the key, least significant first: the hash alone (pair -1), or the seven pairs of key words
    for (int pair = exact ? 6 : -1; pair >= (exact ? 0 : -1); --pair) {
        hipLaunchKernelGGL(uniq_digit_kernel, grid_for(n), dim3(UQ_BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.hash,
                           pair, l.kA);
        t = l.tmp_bytes;
        if ((e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, cur, other, n, 0, pair < 0 ? a.hash_bits : 64, s)) != hipSuccess)
            return e;
        std::swap(cur, other);
    }
    hipLaunchKernelGGL(uniq_boundary_kernel, grid_for(n), dim3(UQ_BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.kB, l.tw,
                       a.ch_bits, a.window, exact ? 1 : 0, l.head, l.info);
    t = l.tmp_bytes;
    if ((e = rocprim::inclusive_scan(l.tmp, t, l.head, l.cid, n, rocprim::plus<uint32_t>(), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_members_kernel, grid_for(n), dim3(UQ_BLOCK), 0, s, a.n_tail, frames, m, cur, l.head, l.cid,
                       l.start, l.prim, l.info);
    // kA / kB are free again: the primaries' output words and their sorted copy
    hipLaunchKernelGGL(uniq_clusters_kernel, grid_for(n), dim3(UQ_BLOCK), 0, s, tail, a.n_tail, frames, m, cur, l.tw,
                       a.ch_bits, a.window, a.rows, l.start, l.prim, l.info, l.kA, l.pent, l.pcopies, l.pidx,
                       static_cast<uint32_t *>(a.tail_out));
    return hipGetLastError();
}

hipError_t unique_deliver_enqueue(const UniqueLaunch &a, int n_primaries, hipStream_t s)
{
    const int m = a.n_tail + a.have;
    if (n_primaries <= 0) return hipSuccess;
    if (n_primaries > a.have || !a.out_frames || !a.out_times || !a.out_copies) return hipErrorInvalidValue;
    const Layout l = carve(a.scratch, a.scratch_bytes, (size_t) m);
    size_t t = l.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(l.tmp, t, l.kA, l.kB, l.pidx, l.pidx2, (size_t) n_primaries, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_gather_kernel, grid_for(4 * (size_t) n_primaries), dim3(UQ_BLOCK), 0, s,
                       static_cast<const uint32_t *>(a.frames), reinterpret_cast<const long long *>(a.times), n_primaries,
                       l.pidx2, l.pent, l.pcopies, reinterpret_cast<uint32_t *>(a.out_frames),
                       reinterpret_cast<long long *>(a.out_times), a.out_copies);
    if (!a.out_first) return hipGetLastError();
    // the member lists: first = the running sum of the copies in output order; then every member of a delivered
    // cluster finds its cluster's list through the primary's ring slot
    if (!a.out_members || (reinterpret_cast<uintptr_t>(a.out_members) & 15u) || !a.heard_scratch ||
        a.heard_scratch_bytes < unique_heard_scratch_bytes(a.have))
        return hipErrorInvalidValue;
    uint32_t *slot2q = static_cast<uint32_t *>(a.heard_scratch), *first = reinterpret_cast<uint32_t *>(a.out_first);
    t = l.tmp_bytes;
    e = rocprim::inclusive_scan(l.tmp, t, reinterpret_cast<const uint32_t *>(a.out_copies), first + 1, (size_t) n_primaries,
                                rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uniq_slot2q_kernel, grid_for((size_t) n_primaries), dim3(UQ_BLOCK), 0, s, n_primaries, l.pidx2, l.pent,
                       slot2q, first);
    // the sorted index array is idxA in both attempts: one sort into idxB, then one (hashed) or seven (exact) more
    hipLaunchKernelGGL(uniq_heard_kernel, grid_for((size_t) m), dim3(UQ_BLOCK), 0, s, a.n_tail,
                       static_cast<const uint32_t *>(a.frames), reinterpret_cast<const long long *>(a.times),
                       static_cast<const u64 *>(a.signal), m, l.idxA, l.cid, l.start, l.prim, slot2q, first,
                       reinterpret_cast<u64 *>(a.out_members));
    return hipGetLastError();
}

} // namespace gnuais
