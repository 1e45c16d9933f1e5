// hdlc_repair.h -- one trial of the single-symbol repair (definition: include/gnuais_hip.h, gnuais_batch_repair).
// The one statement of the trial: the kernel (hdlc_repair.hip) and the host's gnuais_repair_candidate
// (hdlc_repair.cpp) both call these.  Plain C++ for host and device; no HIP needed to include it.
//
// A candidate's raw bits r[0 .. rawlen) lie LSB first in 32-bit words, stuffed 0s included, up to and including the
// fifth 1 of the closing flag.  Trial p inverts bits p and p + 1 and runs ST_DATA of the reference (protodec.c:995-1027)
// over the result, followed by one more 1.  Inside ST_DATA the machine does three things only: it drops the bit behind
// five 1s when that bit is 0, it leaves for ST_STOPSIGN when that bit is 1, and it gives up at 449 stored bits.  So
//   * six 1s in a row anywhere in r' end the frame before the appended bit: not well formed;
//   * otherwise every run of 1s is at most five long, the bits to drop are exactly the 0s behind five 1s (as K3 removes
//     them, a word at a time), and the appended 1 reaches ST_STOPSIGN iff r' ends in five 1s;
//   * bufferpos = rawlen - (stuffed 0s), and it must stay below 449.
// trial_shape() decides all that and gives n'; trial_crc() is K3's CRC over n'/8 + 2 bytes of the unstuffed bits, and
// hands out the payload bytes when asked to.
//
// The repair of long frames (gnuais_batch_long_repair: hdlc_long_repair.hip, hdlc_long_repair.cpp) is the same trial over
// D''s record with D''s numbers, so the four numbers are a parameter of the text, `Limits`: the raw words of a record,
// the most stored bits, the most CRC bytes and the smallest n'.  The default, ShortLimits, is the chain's.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define REPAIR_HD __host__ __device__ inline
#else
#define REPAIR_HD inline
#endif

namespace gnuais {
namespace repair {

struct ShortLimits {
    static constexpr int RAW_WORDS = 18;        // CAND_WORDS - CAND_HDR (kernels.h): the raw words of a candidate record
    static constexpr int RAW_BITS = RAW_WORDS * 32;     // the record's limit
    static constexpr int MAX_STORED = 448;      // bufferpos >= 449 gives the frame up (protodec.c:1024)
    static constexpr int MAX_CRC_BYTES = 60;    // K3 reads no further (HDLC_BUF_WORDS words)
    static constexpr int MIN_BITS = 1;          // n' > 0
};
struct LongLimits {
    static constexpr int RAW_WORDS = 40;        // LONG_REC_WORDS (kernels.h): D''s open record
    static constexpr int RAW_BITS = RAW_WORDS * 32;
    static constexpr int MAX_STORED = 1030;     // D' gives the frame up at 1031 stored bits; n' <= 1008 says the same
    static constexpr int MAX_CRC_BYTES = 128;   // 1008 / 8 + 2
    static constexpr int MIN_BITS = 427;        // n' > 426: at most 426 bits are the chain's decoder's
};
constexpr int RAW_WORDS = ShortLimits::RAW_WORDS, RAW_BITS = ShortLimits::RAW_BITS;
constexpr int MAX_STORED = ShortLimits::MAX_STORED, MAX_CRC_BYTES = ShortLimits::MAX_CRC_BYTES;
constexpr uint32_t CRC_GOOD = 0xf0b8u;      // ~crc == 0x0f47 (protodec.c:166)
constexpr uint32_t POLY = 0x8408u;          // protodec.c:113

REPAIR_HD int popc32(uint32_t v) { return __builtin_popcount(v); }
REPAIR_HD int clz32(uint32_t v) { return __builtin_clz(v); }     // v != 0

// entry b of the byte-wise table: eight steps of protodec.c:111-115 on the byte value
REPAIR_HD uint16_t crc_table_entry(uint32_t b)
{
    for (int k = 0; k < 8; ++k) b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
    return (uint16_t) b;
}

// word q of r': the raw word with the pair at p inverted (p < 0: r itself)
REPAIR_HD uint32_t trial_word(const uint32_t *raw, int q, int p)
{
    uint32_t w = raw[q];
    if (p >= 0) {
        const unsigned long long m = 3ull << (p & 31);
        const int qp = p >> 5;
        if (q == qp) w ^= (uint32_t) m;
        else if (q == qp + 1) w ^= (uint32_t) (m >> 32);
    }
    return w;
}

// bit i = the five bits below bit i of w are all 1, across the word boundary through the previous word
REPAIR_HD uint32_t five_below(uint32_t w, uint32_t prevw)
{
    const unsigned long long cc = ((unsigned long long) w << 32) | prevw;
    return (uint32_t) (cc >> 31) & (uint32_t) (cc >> 30) & (uint32_t) (cc >> 29) & (uint32_t) (cc >> 28) &
           (uint32_t) (cc >> 27);
}

REPAIR_HD uint32_t low_bits(int k) { return k >= 32 ? ~0u : (1u << k) - 1u; }     // k in [0, 32]

// n' of trial p when it is well formed (>= MIN_BITS, a multiple of 8), else -1.  0 < rawlen <= RAW_BITS.
template <class Limits = ShortLimits>
REPAIR_HD int trial_shape(const uint32_t *raw, int rawlen, int p)
{
    if (rawlen < 5 || rawlen > Limits::RAW_BITS) return -1;
    const int nwords = (rawlen + 31) >> 5;
    uint32_t prevw = 0, w = 0, before = 0;
    int stuffed = 0;
    for (int q = 0; q < nwords; ++q) {
        before = prevw;
        w = trial_word(raw, q, p);
        const uint32_t vm = low_bits(rawlen - 32 * q);
        const uint32_t five = five_below(w, prevw) & vm;
        if (five & w) return -1;                    // a sixth 1: ST_STOPSIGN before the appended bit
        stuffed += popc32(five & ~w);
        prevw = w;
    }
    // the appended 1 must find bitstuff set: r' ends in five 1s
    const int e = rawlen - 32 * (nwords - 1);       // bits of the last word, 1..32
    const unsigned long long cc = ((unsigned long long) w << 32) | before;
    if (((cc >> (27 + e)) & 31ull) != 31ull) return -1;
    const int stored = rawlen - stuffed;            // bufferpos at the stop
    if (stored > Limits::MAX_STORED) return -1;
    const int n = stored - 6 - 16;                  // protodec.c:1096
    if (n < Limits::MIN_BITS || (n & 7)) return -1;
    return n;
}

// K3's CRC of trial p over `buflen` bytes of the unstuffed bits (packed LSB first, protodec.c:138-143; zeros behind
// the last bit), before the final complement; the first n_out of those bytes go to out[] (n_out = 0: none).  The
// caller has made sure that r' holds no run of six 1s (trial_shape, or a record the deframer closed).
template <class Limits = ShortLimits>
REPAIR_HD uint32_t trial_crc(const uint32_t *raw, int rawlen, int p, int buflen, const uint16_t *tab, uint8_t *out,
                             int n_out)
{
    if (buflen > Limits::MAX_CRC_BYTES) buflen = Limits::MAX_CRC_BYTES;
    const int nwords = (rawlen + 31) >> 5;
    unsigned long long acc = 0;
    uint32_t prevw = 0, crc = 0xffffu;
    int fill = 0, nbyte = 0;
    for (int q = 0; q < nwords && nbyte < buflen; ++q) {
        uint32_t w = trial_word(raw, q, p);
        const int nvq = rawlen - 32 * q < 32 ? rawlen - 32 * q : 32;
        uint32_t stf = five_below(w, prevw) & ~w & low_bits(nvq);
        prevw = w;
        int nout = nvq;
        while (stf) {                               // highest first: lower positions stay valid
            const int pz = 31 - clz32(stf);
            stf &= ~(1u << pz);
            w = (w & ((1u << pz) - 1u)) | ((pz >= 31 ? 0u : w >> (pz + 1)) << pz);
            --nout;
        }
        w &= low_bits(nout);
        acc |= (unsigned long long) w << fill;      // fill <= 7 here
        fill += nout;
        while (fill >= 8 && nbyte < buflen) {
            const uint32_t byte = (uint32_t) acc & 0xffu;
            if (nbyte < n_out) out[nbyte] = (uint8_t) byte;
            crc = (crc >> 8) ^ tab[(crc ^ byte) & 0xffu];
            acc >>= 8;
            fill -= 8;
            ++nbyte;
        }
    }
    for (; nbyte < buflen; ++nbyte) {               // the stored bits ran out: zeros, as K3's buffer holds them
        const uint32_t byte = (uint32_t) acc & 0xffu;
        if (nbyte < n_out) out[nbyte] = (uint8_t) byte;
        crc = (crc >> 8) ^ tab[(crc ^ byte) & 0xffu];
        acc >>= 8;
    }
    return crc;
}

// trial p passes: well formed and the CRC holds; *n = n'
template <class Limits = ShortLimits>
REPAIR_HD bool trial_passes(const uint32_t *raw, int rawlen, int p, const uint16_t *tab, int *n)
{
    const int n1 = trial_shape<Limits>(raw, rawlen, p);
    if (n1 <= 0) return false;
    *n = n1;
    return trial_crc<Limits>(raw, rawlen, p, (n1 >> 3) + 2, tab, nullptr, 0) == CRC_GOOD;
}

} // namespace repair
} // namespace gnuais
