// resample_plan_main.cpp -- gnuais_amd/csrc/resample_plan.cpp (the wide stage's host planning: plain C++, no GPU) on the
// CPU under ASan + UBSan, built and run by tests/test_resampler_cpu.py.  For each "up down" pair on the command line:
// the default prototype, its checks and its tables at the fast form's 17 accumulators, and the invariants of the
// tables; prints one line per ratio.  "poly K D T": the integer channeliser's plan for K offsets, decimation D and the
// T taps h[j] = (j * 7919 + 13) % 4001 - 2000 -- a line "NA n_pairs", then the pair table, one row of NA words per line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "resample_plan.h"

using namespace gnuais;

static int fail(const char *what, int up, int down)
{
    fprintf(stderr, "%d/%d: %s\n", up, down, what);
    return 1;
}

static int poly(int K, int D, int T)
{
    std::vector<int16_t> h((size_t) T);
    for (int j = 0; j < T; ++j) h[(size_t) j] = (int16_t) ((j * 7919 + 13) % 4001 - 2000);
    const int na = channeliser_fast_na(K, T, D);
    ResamplePlan p;
    if (na) resample_plan(1, D, h.data(), T, na, p);
    printf("%d %d\n", na, p.n_pairs);
    for (int q = 0; q < p.n_pairs; ++q)
        for (int a = 0; a < na; ++a) printf("%u%c", p.pairs[(size_t) q * (size_t) na + (size_t) a], a + 1 < na ? ' ' : '\n');
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "poly")) return poly(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    for (int a = 1; a + 1 < argc; a += 2) {
        const int up = atoi(argv[a]), down = atoi(argv[a + 1]);
        if (resample_check_ratio(up, down)) return fail("ratio refused", up, down);
        std::vector<int16_t> h;
        resample_default_taps(up, down, h);
        const int T = (int) h.size();
        if (resample_check_taps(up, h.data(), T)) return fail("default taps refused", up, down);
        const int na = resampler_fast_na(2, T, down);
        if (na != RESAMP_FAST_NA) return fail("no fast form for the default design", up, down);
        ResamplePlan p;
        resample_plan(up, down, h.data(), T, na, p);
        long long sizes = 0, seen = 0, taps_sum = 0, table_sum = 0;
        for (int i = 0; i < up; ++i) {
            const ResampGroup &g = p.groups[(size_t) i];
            if (i && g.first <= p.groups[(size_t) i - 1].first) return fail("first[] not increasing", up, down);
            sizes += g.size;
        }
        if (sizes != down) return fail("group sizes do not sum to down", up, down);
        for (uint32_t w : p.pairs) {
            const int lo = (int16_t) (w & 0xffffu), hi = (int16_t) (w >> 16);
            seen += (lo != 0) + (hi != 0);
            table_sum += lo + hi;
        }
        long long nonzero = 0;
        for (int16_t v : h) { nonzero += v != 0; taps_sum += v; }
        if (seen != nonzero || table_sum != taps_sum) return fail("the pair table does not hold every tap once", up, down);
        printf("%d/%d T %d NA %d H %d pairs %d\n", up, down, T, p.NA, p.H, p.n_pairs);
    }
    // the refusals
    if (resample_check_ratio(0, 3) != 1 || resample_check_ratio(65, 128) != 1 || resample_check_ratio(3, 1025) != 2 ||
        resample_check_ratio(3, 3) != 3 || resample_check_ratio(6, 5) != 3 || resample_check_ratio(6, 128) != 4)
        return fail("ratio checks", 0, 0);
    const int16_t at[4] = {32767, 1, 32767, 32767}, over[4] = {32767, 0, 32767, 2}, neg[1] = {-32768};
    if (resample_check_taps(2, at, 4) != 0 || resample_check_taps(1, at, 4) != 3 || resample_check_taps(2, over, 4) != 0 ||
        resample_check_taps(1, neg, 1) != 2 || resample_check_taps(2, at, 0) != 1)
        return fail("tap checks", 0, 0);
    return 0;
}
