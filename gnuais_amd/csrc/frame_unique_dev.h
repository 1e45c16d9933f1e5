// frame_unique_dev.h -- how the device stage of the duplicate merge (frame_unique.hip) reads and writes a record: one
// policy per kind of record over the traits of frame_unique.h, holding what differs between the two and nothing else.
// Included by frame_unique.hip alone.
//
// ShortDev  gnuais_frame: 16 32-bit words, 16-byte aligned, read and moved as four 16-byte quarters.  The member time is
//           times[ring slot]; a tail entry is [t_last (words 0..1) | key (words 2..15, the last one masked)].
// LongDev   gnuais_long_frame: 152 bytes, 8-byte aligned only, so every access is in 64-bit words, 19 per record: word 0
//           channel | end_bit << 32, word 1 t, word 2 nbits | flags << 16 | reserved << 24 | payload[0..3] << 32, words
//           3..18 the rest of the payload.  The key is words 2..18 with word 2 masked: the 17 pairs of the definition.  The
//           member time is the record's own word 1, and a tail entry is a record with t_last there and word 2 masked.
//
// Both answer: word / WORDS (a record in memory), Image and load (a record in registers), PAIRS and pair(w, p) (the key
// as 64-bit digits, from memory or from an image), tail_time / frame_time, channel, repaired_bit, stamp37, flags (of a
// record in memory), chunk / CHUNKS (what one thread of the gather moves), MEMBER_ALIGN and store_hearer, TAIL_BY_WORDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_unique.h"

namespace gnuais {

typedef unsigned long long u64;

struct ShortDev : uniq::ShortRec {
    typedef uint32_t word;
    typedef uint4 chunk;
    static constexpr int WORDS = 16, PAIRS = 7, CHUNKS = 4, MEMBER_ALIGN = 16;
    static constexpr bool TAIL_BY_WORDS = false;        // the clusters kernel writes a tail entry itself, from an image
    struct Image { uint32_t w[16]; };
    static __device__ __forceinline__ Image load(const uint32_t *rec)
    {
        Image r;
        const uint4 *q = reinterpret_cast<const uint4 *>(rec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = q[k];
            r.w[4 * k] = v.x; r.w[4 * k + 1] = v.y; r.w[4 * k + 2] = v.z; r.w[4 * k + 3] = v.w;
        }
        return r;
    }
    static __device__ __forceinline__ u64 pair(const uint32_t *w, int p)
    {
        return (u64) key_word(w, 2 * p) | ((u64) key_word(w, 2 * p + 1) << 32);
    }
    static __device__ __forceinline__ long long tail_time(const uint32_t *w) { return (long long) ((u64) w[0] | ((u64) w[1] << 32)); }
    static __device__ __forceinline__ long long frame_time(const uint32_t *, const long long *times, uint32_t slot) { return times[slot]; }
    static __device__ __forceinline__ uint32_t channel(const uint32_t *w) { return w[0]; }
    // the first entry of a cluster that stays open, as the next drain's tail entry
    static __device__ __forceinline__ void store_tail(uint32_t *out, Image r, long long t_last)
    {
        r.w[0] = (uint32_t) ((u64) t_last & 0xffffffffull);
        r.w[1] = (uint32_t) ((u64) t_last >> 32);
        r.w[15] &= uniq::KEY_LAST_MASK;
        uint4 *q = reinterpret_cast<uint4 *>(out);
#pragma unroll
        for (int x = 0; x < 4; ++x) q[x] = make_uint4(r.w[4 * x], r.w[4 * x + 1], r.w[4 * x + 2], r.w[4 * x + 3]);
    }
    // 24 bytes per member at 24 * pos, the lists 16-byte aligned: the 16-byte store takes whichever half is 16-aligned
    static __device__ __forceinline__ void store_hearer(u64 *out, size_t pos, uint32_t channel, uint32_t flags, long long t, u64 sig)
    {
        const uint32_t t_lo = (uint32_t) ((u64) t & 0xffffffffull), t_hi = (uint32_t) ((u64) t >> 32);
        if ((pos & 1) == 0) {
            *reinterpret_cast<uint4 *>(out) = make_uint4(channel, flags, t_lo, t_hi);
            out[2] = sig;
        } else {
            out[0] = (u64) channel | ((u64) flags << 32);
            *reinterpret_cast<uint4 *>(out + 1) = make_uint4(t_lo, t_hi, (uint32_t) (sig & 0xffffffffull), (uint32_t) (sig >> 32));
        }
    }
};

struct LongDev : uniq::LongRec {
    typedef u64 word;
    typedef u64 chunk;
    static constexpr int WORDS = REC_WORDS64, PAIRS = KEY_PAIRS, CHUNKS = REC_WORDS64, MEMBER_ALIGN = 8;
    static constexpr bool TAIL_BY_WORDS = true;         // the clusters kernel notes the entry, the tail kernel copies it
    struct Image { u64 w[REC_WORDS64]; };
    static __device__ __forceinline__ Image load(const u64 *rec)
    {
        Image r;
#pragma unroll
        for (int k = 0; k < REC_WORDS64; ++k) r.w[k] = rec[k];
        return r;
    }
    static __device__ __forceinline__ u64 pair(const u64 *w, int p) { return key_word64(w[KEY_WORD64 + p], p); }
    static __device__ __forceinline__ long long tail_time(const u64 *w) { return (long long) w[T_WORD64]; }
    static __device__ __forceinline__ long long frame_time(const u64 *w, const long long *, uint32_t) { return (long long) w[T_WORD64]; }
    static __device__ __forceinline__ uint32_t channel(const u64 *w) { return (uint32_t) w[0]; }
    static __device__ __forceinline__ uint32_t repaired_bit(const u64 *w) { return repaired_bit64(w[KEY_WORD64]); }
    static __device__ __forceinline__ u64 stamp37(const u64 *w) { return stamp37_64(w[0], w[KEY_WORD64]); }
    static __device__ __forceinline__ uint32_t flags(const u64 *w) { return flags64(w[KEY_WORD64]); }
    // word x of a tail entry, from word x of the cluster's first entry
    static __device__ __forceinline__ u64 tail_word(u64 v, uint32_t x, u64 t_last)
    {
        return x == (uint32_t) T_WORD64 ? t_last : x == (uint32_t) KEY_WORD64 ? v & KEY_FIRST_MASK64 : v;
    }
    static __device__ __forceinline__ void store_hearer(u64 *out, size_t, uint32_t channel, uint32_t flags, long long t, u64 sig)
    {
        out[0] = (u64) channel | ((u64) flags << 32);
        out[1] = (u64) t;
        out[2] = sig;
    }
};

} // namespace gnuais
