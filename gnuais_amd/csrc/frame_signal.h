// frame_signal.h -- the span of a frame in the blocks of the I/Q it was decoded from (definition: include/gnuais_hip.h,
// gnuais_batch_frame_signal): which whole blocks of 64 rows lie inside [q - S, q] and whether the record is valid.  One
// text for the host (frame_signal.cpp: gnuais_frame_signal_span, the ring's size) and the device (frame_signal.hip:
// frame_signal_kernel), so the two cannot drift apart.  Plain integer arithmetic, no HIP.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_HD __host__ __device__
#else
#define FS_HD
#endif

namespace gnuais {

constexpr int FS_BLOCK = 64;            // rows of a block of n
constexpr int FS_MAX_NBITS = 448;       // the longest frame the deframer delivers (449 stored bits give up)
constexpr int FS_LONG_MAX_NBITS = 1008; // the longest frame of gnuais_batch_long_frames (GNUAIS_LONG_MAX_BITS)

// floor(a / b) and ceil(a / b) for b > 0 and any a
FS_HD inline long long fs_floor_div(long long a, long long b) { return a / b - (a % b < 0 ? 1 : 0); }
FS_HD inline long long fs_ceil_div(long long a, long long b) { return a / b + (a % b > 0 ? 1 : 0); }

// S: payload, CRC and closing flag at the nominal bit length, in rows
FS_HD inline long long fs_span_rows(int nbits, uint32_t pllinc)
{
    return ((long long) nbits + 24) * 65536 / (long long) pllinc;
}

// The whole blocks inside [q - S, q] of a frame with time t: [*j_lo, *j_lo + *nb).  Returns false, with *j_lo = 0 and
// *nb = 0, where the record is (0, 0, 0): t < 0, no whole block, or a span that reaches behind v0.  pllinc > 0.
FS_HD inline bool fs_span(long long t, int nbits, uint32_t pllinc, int n_taps, int afc_window, long long v0,
                          long long *j_lo, int *nb)
{
    *j_lo = 0;
    *nb = 0;
    if (t < 0) return false;
    const long long q = t - (n_taps + 1) / 2 - afc_window / 2;
    const long long lo = fs_ceil_div(q - fs_span_rows(nbits, pllinc), FS_BLOCK);
    const long long n = fs_floor_div(q + 1, FS_BLOCK) - lo;
    if (n <= 0 || lo * FS_BLOCK < v0) return false;
    *j_lo = lo;
    *nb = (int) n;
    return true;
}

} // namespace gnuais
