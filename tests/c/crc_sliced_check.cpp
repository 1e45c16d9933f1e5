// crc_sliced_check.cpp -- gnuais_amd/csrc/crc_sliced.h (the text K3 runs) as a small shared library for
// tests/test_crc_sliced_cpu.py: the four tables as the header builds them, the register after n bytes taken four at a
// time (run_words), and the same bytes one at a time through table 0.  Plain C++, no HIP.
#include <string.h>

#include "../../gnuais_amd/csrc/crc_sliced.h"

using namespace gnuais::crc;

namespace {
struct Tables {
    uint16_t t[SLICES * 256];
    Tables()
    {
        // as the kernel fills its LDS copy: entry b of table k from entry b of table k-1
        for (uint32_t b = 0; b < 256; ++b) {
            uint32_t v = b;
            for (int k = 0; k < SLICES; ++k) {
                v = advance8(v);
                t[k * 256 + b] = (uint16_t) v;
            }
        }
    }
};
const Tables tab;
}

extern "C" {

int crc_sliced_slices(void) { return SLICES; }

void crc_sliced_tables(uint16_t *out) { memcpy(out, tab.t, sizeof tab.t); }

// the header's closed form of one entry
unsigned crc_sliced_entry(int k, unsigned b) { return sliced_entry(k, b); }

// the register (no final complement) after n bytes, from 0xffff: whole words by step4, the tail by bytes
unsigned crc_sliced_run(const uint8_t *data, int n)
{
    uint32_t w[32] = {0};
    if (n < 0 || n > (int) sizeof w) return ~0u;
    for (int i = 0; i < n; ++i) w[i >> 2] |= (uint32_t) data[i] << (8 * (i & 3));
    return run_words(0xffffu, w, n, tab.t);
}

// the same, a byte at a time
unsigned crc_sliced_bytewise(const uint8_t *data, int n)
{
    uint32_t crc = 0xffffu;
    for (int i = 0; i < n; ++i) crc = step1(crc, data[i], tab.t);
    return crc;
}

} // extern "C"
