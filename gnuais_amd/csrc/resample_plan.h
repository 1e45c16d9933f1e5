// resample_plan.h -- what the host decides before the wide stage (wide_kernels.h) can run, at an integer ratio (U = 1,
// gnuais_batch_channeliser) and at a rational one (gnuais_batch_resampler): the default prototype, the checks of a
// prototype, the fast form's accumulators and the two tables it reads.  Everything here depends on (U, D, T, taps) alone.  Plain C++, no HIP: resample_plan.cpp is also built for the CPU under ASan + UBSan by
// tests/test_resampler_cpu.py (tests/c/resample_plan_main.cpp), like fir_plan.cpp.  The definition is in
// include/gnuais_hip.h above gnuais_batch_resampler.
//
// With out rate = in rate * U / D, narrowband row m ends on up-sampled tick u_m = m*D + D-1, and wide sample n sits on
// tick n*U.  Sample n belongs to GROUP g when g*D <= n*U < (g+1)*D: the samples that arrive between the ends of rows
// g-1 and g.  It feeds rows g + a, a = 0 .. NA-1 (NA = ceil(T / D)), with tap j = (g + a)*D + D-1 - n*U.  Groups repeat
// with period U rows = D samples: for g = c*U + i the first sample is c*D + first[i] and the taps depend on i alone.
// At U = 1 there is one group, the D samples from g*D on, and the pair table is the integer channeliser's
// POLY[q][a] = (h[aD + D-1-2q], h[aD + D-2-2q]).
#pragma once
#include <stdint.h>

#include <vector>

namespace gnuais {

constexpr int RESAMP_MAX_UP = 64, RESAMP_MAX_DOWN = 1024, RESAMP_MAX_TAPS = 16385;
constexpr int RESAMP_FAST_NA = 17;   // the fast form's one bucket of accumulators per offset

// row phase i of the period: its first wide sample relative to the period, its size, its first pair in the pair table
struct ResampGroup { int32_t first, size, base; };

struct ResamplePlan {
    int U = 0, D = 0, T = 0;
    int NA = 0;                       // the pair table's accumulators per row: the `na` it was planned with, >= ceil(T / D)
    int H = 0;                        // ceil((T - 1) / U): the carry, in wide samples per stream
    int n_pairs = 0;                  // sum over i of ceil(size_i / 2)
    std::vector<ResampGroup> groups;  // [U]
    // [n_pairs][NA] words (tap of sample k lo, tap of sample k + 1 hi): pair q of phase i, accumulator a, at
    // (groups[i].base + q) * NA + a; a tap index outside [0, T) and the missing partner of an odd group's last sample: 0
    std::vector<uint32_t> pairs;
};

// 0, or the first limit (up, down) breaks: 1 up range, 2 down range, 3 up >= down, 4 gcd != 1
int resample_check_ratio(int up, int down);
// the default prototype for (up, down): T = 16*down + 1 taps
void resample_default_taps(int up, int down, std::vector<int16_t> &h);
// 0, or why the prototype is refused: 1 count, 2 a tap of -32768, 3 a phase's sum |h| above 65535
int resample_check_taps(int up, const int16_t *h, int T);
// the tables with `na` accumulators per row in the pair table (na >= ceil(T / D), the rows a wide sample feeds; the
// surplus holds zeros); p.NA = na
void resample_plan(int up, int down, const int16_t *h, int T, int na, ResamplePlan &p);
// the fast form's accumulators per offset for this shape (RESAMP_FAST_NA), 0 = the direct form
int resampler_fast_na(int K, int T, int D);
// the same for gnuais_batch_channeliser, whose fast form has more buckets: 4, 8, 17, and 33 for K <= 2
int channeliser_fast_na(int K, int T, int D);

} // namespace gnuais
