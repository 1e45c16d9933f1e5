// crc_sliced.h -- the reference's CRC (protodec_sdlc_crc(), src/protodec.c:106-118: CRC-16/X-25's register, reflected,
// polynomial 0x8408, one LFSR step per bit, bytes LSB first) taken four bytes per dependent step.
//
// Table k, entry b = the register 8 * (k + 1) LFSR steps after it held b: table 0 is the byte table everybody uses
// (crc' = (crc >> 8) ^ T0[(crc ^ byte) & 0xff]), table k is table k-1 moved on by one zero byte.  The register is 16 bits
// wide, so after two bytes nothing of the old register is left but what the look-ups carry, and four bytes b0..b3 cost
// one round of four independent look-ups:
//     v = crc ^ (b0 | b1 << 8 | b2 << 16 | b3 << 24);  crc' = T3[v & 0xff] ^ T2[v >> 8 & 0xff] ^ T1[v >> 16 & 0xff] ^ T0[v >> 24]
// Every entry is built from the bitwise definition, as K3's byte table always was.  The text K3 runs (hdlc_crc.hip) and the
// text the CPU test runs (tests/test_crc_sliced_cpu.py) are this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace gnuais {
namespace crc {

constexpr uint32_t POLY = 0x8408u;
constexpr int SLICES = 4;

// eight steps of the LFSR: a table's entry from the same entry of the table before it (table 0's from the byte value)
CRC_HD uint32_t advance8(uint32_t b)
{
    for (int s = 0; s < 8; ++s) b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
    return b;
}

// entry b of table k: 8 * (k + 1) steps on the byte value
CRC_HD uint16_t sliced_entry(int k, uint32_t b)
{
    for (int s = 0; s <= k; ++s) b = advance8(b);
    return (uint16_t) b;
}

// one byte (tab = table 0)
CRC_HD uint32_t step1(uint32_t crc, uint32_t byte, const uint16_t *tab)
{
    return (crc >> 8) ^ tab[(crc ^ byte) & 0xffu];
}

// four bytes, the first in the word's low byte (tab = the four tables, 256 entries each, table 0 first)
CRC_HD uint32_t step4(uint32_t crc, uint32_t word, const uint16_t *tab)
{
    const uint32_t v = crc ^ word;
    return (uint32_t) tab[3 * 256 + (v & 0xffu)] ^ (uint32_t) tab[2 * 256 + ((v >> 8) & 0xffu)] ^
           (uint32_t) tab[256 + ((v >> 16) & 0xffu)] ^ (uint32_t) tab[v >> 24];
}

// the register after the first n bytes of w[] (little-endian words), from crc: whole words by step4, the tail by bytes
CRC_HD uint32_t run_words(uint32_t crc, const uint32_t *w, int n, const uint16_t *tab)
{
    int q = 0;
    for (; 4 * q + 4 <= n; ++q) crc = step4(crc, w[q], tab);
    for (int k = 4 * q; k < n; ++k) crc = step1(crc, (w[k >> 2] >> (8 * (k & 3))) & 0xffu, tab);
    return crc;
}

} // namespace crc
} // namespace gnuais
