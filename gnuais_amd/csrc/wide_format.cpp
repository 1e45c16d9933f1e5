// wide_format.cpp -- gnuais_sample_format_bytes / gnuais_convert_samples (include/gnuais_hip.h): the sample formats of
// wideband input on the host, from the formulas the kernels use (wide_format.h).  Plain C++, no HIP: built into the
// library with -ffp-contract=off, and by itself with g++ under the sanitizers (tests/test_wide_format_cpu.py).
#include <string.h>

#include "../../include/gnuais_hip.h"
#include "wide_format.h"

static_assert(GNUAIS_FMT_CS16 == gnuais::FMT_CS16 && GNUAIS_FMT_CU8 == gnuais::FMT_CU8 &&
              GNUAIS_FMT_CS8 == gnuais::FMT_CS8 && GNUAIS_FMT_CF32 == gnuais::FMT_CF32, "wide_format.h restates GNUAIS_FMT_*");

extern "C" {

int gnuais_sample_format_bytes(int fmt)
{
    const int n = gnuais::wide_format_bytes(fmt);
    return n ? n : GNUAIS_E_ARG;
}

// `in` may have any alignment (it is read byte-wise); out[2 * n_pairs]
int gnuais_convert_samples(int fmt, const void *in, size_t n_pairs, int16_t *out)
{
    if (!gnuais::wide_format_bytes(fmt) || !in || !out) return GNUAIS_E_ARG;
    const unsigned char *p = (const unsigned char *) in;
    for (size_t i = 0; i < n_pairs; ++i) {
        uint32_t w;
        if (fmt == GNUAIS_FMT_CS16) {
            memcpy(&w, p + 4 * i, 4);
        } else if (fmt == GNUAIS_FMT_CF32) {
            float x[2];
            memcpy(x, p + 8 * i, 8);
            w = gnuais::wide_word_cf32(x[0], x[1]);
        } else {
            const uint32_t pair = (uint32_t) p[2 * i] | (uint32_t) p[2 * i + 1] << 8;
            w = fmt == GNUAIS_FMT_CU8 ? gnuais::wide_word_cu8(pair) : gnuais::wide_word_cs8(pair);
        }
        out[2 * i] = (int16_t) (uint16_t) (w & 0xffffu);
        out[2 * i + 1] = (int16_t) (uint16_t) (w >> 16);
    }
    return GNUAIS_OK;
}

} // extern "C"
