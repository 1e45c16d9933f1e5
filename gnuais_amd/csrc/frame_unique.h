// frame_unique.h -- what the host objects (frame_unique.cpp) and the device stage (frame_unique.hip, through the record
// policies of frame_unique_dev.h) of the duplicate merge share: how a record's key, repaired bit, 37-bit stamp and time
// are read -- one traits type per kind of record, ShortRec (gnuais_frame) and LongRec (gnuais_long_frame) -- and the sort
// words of the definition (include/gnuais_hip.h, gnuais_batch_unique and gnuais_batch_long_unique).  Plain C++, no HIP;
// internal to csrc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GNUAIS_UQ_HD __host__ __device__ inline
#else
#define GNUAIS_UQ_HD inline
#endif

namespace gnuais {
namespace uniq {

// A record is 16 words: [0] channel, [1] end_bit, [2..14] payload bytes 0..51, [15] payload[52] | flags << 8 | nbits << 16.
// The key is nbits and the 53 payload bytes: words 2..14 and word 15 without its flags byte.
constexpr int KEY_WORDS = 14;
constexpr uint32_t KEY_LAST_MASK = 0xffff00ffu;
constexpr int CHANNEL_BITS = 24;                // channels below 2^24, rows below 2^39: one 64-bit sort word

GNUAIS_UQ_HD uint32_t key_word(const uint32_t *rec, int k)      // k in [0, KEY_WORDS)
{
    return k < KEY_WORDS - 1 ? rec[2 + k] : rec[15] & KEY_LAST_MASK;
}
GNUAIS_UQ_HD uint32_t repaired_bit(const uint32_t *rec) { return (rec[15] >> 14) & 1u; }     // flags bit 6
GNUAIS_UQ_HD uint64_t stamp37(const uint32_t *rec) { return (uint64_t) rec[1] | ((uint64_t) ((rec[15] >> 9) & 31u) << 32); }

// member order inside a key, and the output order of the timed primaries: (t, channel), t >= 0
GNUAIS_UQ_HD uint64_t time_word(long long t, uint32_t channel)
{
    return ((uint64_t) (t + 1) << CHANNEL_BITS) | (uint64_t) (channel & ((1u << CHANNEL_BITS) - 1u));
}
// output order over everything: the untimed frames first, by (channel, stamp) as the plain drain orders them, then
// the timed ones by (t, channel)
GNUAIS_UQ_HD uint64_t output_word(long long t, uint32_t channel, uint64_t stamp)
{
    return t < 0 ? ((uint64_t) (channel & ((1u << CHANNEL_BITS) - 1u)) << 37) | stamp : (1ull << 63) | time_word(t, channel);
}

// ---- the record-dependent parts of the merge, one type per kind of record ----
// REC_WORDS: 32-bit words of a record, and of a tail entry (t_last in the words TAIL_T_WORD, TAIL_T_WORD + 1; the key
// words where a record holds them, the last / first one masked to the key).  key_word(rec, k), k in [0, KEY_WORDS): the
// key; KEY_WORDS is even, the exact path sorts by pairs (2p, 2p + 1).  TIMED_BY_RECORD: the member time is in the record
// (record_time) and not in an array beside the ring.
struct ShortRec {
    static constexpr int REC_WORDS = 16, KEY_WORDS = uniq::KEY_WORDS, TAIL_T_WORD = 0;
    static constexpr bool TIMED_BY_RECORD = false;
    static GNUAIS_UQ_HD uint32_t key_word(const uint32_t *rec, int k) { return uniq::key_word(rec, k); }
    static GNUAIS_UQ_HD uint32_t repaired_bit(const uint32_t *rec) { return uniq::repaired_bit(rec); }
    static GNUAIS_UQ_HD uint64_t stamp37(const uint32_t *rec) { return uniq::stamp37(rec); }
    static GNUAIS_UQ_HD uint32_t flags(const uint32_t *rec) { return (rec[15] >> 8) & 0xffu; }
    static GNUAIS_UQ_HD long long record_time(const uint32_t *) { return -1; }
};

// A long record is 38 words: [0] channel, [1] end_bit, [2..3] t, [4] nbits | flags << 16 | reserved << 24, [5..37] the 132
// payload bytes.  The key is nbits and the payload: word 4 without its upper half and words 5..37 -- 34 words, 17 pairs,
// which are the record's 64-bit words 2..18 with the first one masked (KEY_FIRST_MASK64).
struct LongRec {
    static constexpr int REC_WORDS = 38, KEY_WORDS = 34, TAIL_T_WORD = 2;
    static constexpr int REC_WORDS64 = 19, KEY_WORD64 = 2, KEY_PAIRS = 17, T_WORD64 = 1;
    static constexpr uint32_t KEY_FIRST_MASK = 0x0000ffffu;
    static constexpr uint64_t KEY_FIRST_MASK64 = 0xffffffff0000ffffull;
    static constexpr bool TIMED_BY_RECORD = true;
    static GNUAIS_UQ_HD uint32_t key_word(const uint32_t *rec, int k) { return k ? rec[4 + k] : rec[4] & KEY_FIRST_MASK; }
    static GNUAIS_UQ_HD uint32_t repaired_bit(const uint32_t *rec) { return (rec[4] >> 22) & 1u; }    // flags bit 6
    static GNUAIS_UQ_HD uint64_t stamp37(const uint32_t *rec) { return (uint64_t) rec[1] | ((uint64_t) ((rec[4] >> 17) & 31u) << 32); }
    static GNUAIS_UQ_HD uint32_t flags(const uint32_t *rec) { return (rec[4] >> 16) & 0xffu; }
    static GNUAIS_UQ_HD long long record_time(const uint32_t *rec)
    {
        return (long long) ((uint64_t) rec[2] | ((uint64_t) rec[3] << 32));
    }
    // the same on a record's 64-bit words (the device stage reads records in those: they are 8-byte aligned only)
    static GNUAIS_UQ_HD uint64_t key_word64(uint64_t q, int p) { return p ? q : q & KEY_FIRST_MASK64; }    // q = word 2 + p
    static GNUAIS_UQ_HD uint32_t repaired_bit64(uint64_t q2) { return (uint32_t) (q2 >> 22) & 1u; }
    static GNUAIS_UQ_HD uint64_t stamp37_64(uint64_t q0, uint64_t q2) { return (q0 >> 32) | (((q2 >> 17) & 31u) << 32); }
    static GNUAIS_UQ_HD uint32_t flags64(uint64_t q2) { return (uint32_t) (q2 >> 16) & 0xffu; }
};

} // namespace uniq
} // namespace gnuais
