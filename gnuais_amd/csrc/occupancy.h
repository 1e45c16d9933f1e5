// occupancy.h -- the channel load per receiver (definition: include/gnuais_hip.h, gnuais_batch_occupancy): the code of a
// block's power, the cover span of a frame in blocks of 64 rows, and the rows an epoch has to wait for.  One text for the
// host (occupancy.cpp: gnuais_occupancy_code, _power, _cover_span; capi_ingest.hip: the rings' size and the finality of
// an epoch) and the device (occupancy.hip), so the two cannot drift apart.  Plain integer arithmetic, no HIP.
#pragma once
#include <stdint.h>

#include "frame_signal.h"

namespace gnuais {

constexpr int OCC_BINS = 288;               // codes 0 .. 287: P < 2^38
constexpr int OCC_CODE_MASK = 0x1ff;        // the code in a word of the code ring; bit 14 busy, bit 15 cover once final
constexpr int OCC_BUSY_BIT = 14, OCC_COVER_BIT = 15;
constexpr int OCC_MIN_EPOCH = 64, OCC_MAX_EPOCH = 4096;
constexpr int OCC_RING_EPOCHS = 64;         // final epochs the output ring holds

// code(P), 0 <= P < 2^38: P below 8, else eight steps per octave: 8 (e - 2) + the three bits under the leading one
FS_HD inline int occ_code(long long P)
{
    if (P < 8) return (int) (P < 0 ? 0 : P);
    const int e = 63 - __builtin_clzll((unsigned long long) P);
    return 8 * (e - 2) + (int) ((P >> (e - 3)) & 7);
}

// power(code): the lower edge of the code's bin
FS_HD inline long long occ_power(int code)
{
    return code < 8 ? (long long) code : (long long) (8 + (code & 7)) << (code / 8 - 1);
}

// S_pre and S_post: ramp, training, start flag and stuffing in front of a frame's span, eight bits behind it
FS_HD inline long long occ_pre_rows(uint32_t pllinc) { return 64LL * 65536 / (long long) pllinc; }
FS_HD inline long long occ_post_rows(uint32_t pllinc) { return 8LL * 65536 / (long long) pllinc; }

// LAG: an epoch whose last row is r is final once a call ends behind row r + LAG -- every frame whose cover span
// [q - S - S_pre, q + S_post] can begin at or before r has its time by then (t = q + d_f + W/2 <= r + S + S_pre + d_f + W/2).
// max_nbits: the longest frame that covers -- FS_LONG_MAX_NBITS where the long frames cover too (gnuais_batch_long_frame_signal)
FS_HD inline long long occ_lag_rows(uint32_t pllinc, int n_taps, int afc_window, int max_nbits = FS_MAX_NBITS)
{
    return fs_span_rows(max_nbits, pllinc) + occ_pre_rows(pllinc) + (n_taps + 1) / 2 + afc_window / 2 + FS_BLOCK;
}

// The blocks the cover span of a frame with time t intersects: [*j_lo, *j_lo + *nb).  Returns false, with 0 and 0, where
// the frame covers nothing: t < 0, or a span that begins before v0.  pllinc > 0.
FS_HD inline bool occ_cover_span(long long t, int nbits, uint32_t pllinc, int n_taps, int afc_window, long long v0,
                                 long long *j_lo, int *nb)
{
    *j_lo = 0;
    *nb = 0;
    if (t < 0) return false;
    const long long q = t - (n_taps + 1) / 2 - afc_window / 2;
    const long long lo = q - fs_span_rows(nbits, pllinc) - occ_pre_rows(pllinc), hi = q + occ_post_rows(pllinc);
    if (lo < v0) return false;
    *j_lo = fs_floor_div(lo, FS_BLOCK);
    *nb = (int) (fs_floor_div(hi, FS_BLOCK) - *j_lo + 1);
    return true;
}

} // namespace gnuais
