// frame_unique.h -- what the host object (frame_unique.cpp) and the device stage (frame_unique.hip) of the duplicate
// merge share: how a frame record's key, repaired bit and 37-bit stamp are read, and the sort words of the definition
// (include/gnuais_hip.h, gnuais_batch_unique).  Plain C++, no HIP; internal to csrc.
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

} // namespace uniq
} // namespace gnuais
