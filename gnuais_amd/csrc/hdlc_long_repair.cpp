// hdlc_long_repair.cpp -- gnuais_long_repair_candidate: the single-symbol repair of one long candidate on the host
// (definition: include/gnuais_hip.h, gnuais_batch_long_repair).  The trial is hdlc_repair.h's with LongLimits, the text
// the kernel runs (hdlc_long_repair.hip); here every trial p is taken in turn.  Plain C++, no HIP.
#include "hdlc_repair.h"

#include "../../include/gnuais_hip.h"

using namespace gnuais::repair;

namespace {
struct Table {
    uint16_t t[256];
    Table() { for (uint32_t b = 0; b < 256; ++b) t[b] = crc_table_entry(b); }
};
}

extern "C" int gnuais_long_repair_candidate(const uint8_t *raw_bits, int n_raw, uint8_t payload[126], int *nbits, int *pos)
{
    static const Table tab;
    if (!raw_bits || !payload || !nbits || !pos || n_raw < 0) return GNUAIS_E_ARG;
    if (n_raw < 2 || n_raw > LongLimits::RAW_BITS) return 0;    // no trial, or more than the 40 words hold
    uint32_t raw[LongLimits::RAW_WORDS] = {0};
    for (int i = 0; i < n_raw; ++i) raw[i >> 5] |= (uint32_t) (raw_bits[i] & 1u) << (i & 31);
    int passing = 0, p1 = -1, n1 = 0;
    for (int p = 0; p <= n_raw - 2; ++p) {
        int n = 0;
        if (trial_passes<LongLimits>(raw, n_raw, p, tab.t, &n)) {
            if (!passing) { p1 = p; n1 = n; }
            ++passing;
        }
    }
    if (passing == 1) {
        for (int j = 0; j < 126; ++j) payload[j] = 0;
        (void) trial_crc<LongLimits>(raw, n_raw, p1, (n1 >> 3) + 2, tab.t, payload, n1 >> 3);
        *nbits = n1;
        *pos = p1;
    }
    return passing;
}
