// resample_plan.cpp -- the wide stage's host planning (resample_plan.h).  Plain C++.
#include "resample_plan.h"

#include <math.h>
#include <stdlib.h>

namespace gnuais {

static int gcd_int(int a, int b)
{
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// floor(a / b) for b > 0, also for a < 0
static int floor_div(int a, int b)
{
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

int resample_check_ratio(int up, int down)
{
    if (up < 1 || up > RESAMP_MAX_UP) return 1;
    if (down < 1 || down > RESAMP_MAX_DOWN) return 2;
    if (up >= down) return 3;
    if (gcd_int(up, down) != 1) return 4;
    return 0;
}

void resample_default_taps(int up, int down, std::vector<int16_t> &h)
{
    const int D = down, T = 16 * D + 1;
    std::vector<double> g((size_t) T);
    double G = 0.0;
    for (int j = 0; j < T; ++j) {
        const double w = 0.42 - 0.5 * cos(2.0 * M_PI * j / (T - 1)) + 0.08 * cos(4.0 * M_PI * j / (T - 1));
        const double x = 0.75 * (j - 8 * D) / D;
        const double s = (x == 0.0) ? 1.0 : sin(M_PI * x) / (M_PI * x);
        g[(size_t) j] = w * s;
        G += g[(size_t) j];
    }
    h.resize((size_t) T);
    for (int j = 0; j < T; ++j) h[(size_t) j] = (int16_t) lround(g[(size_t) j] * 32768.0 * up / G);
}

int resample_check_taps(int up, const int16_t *h, int T)
{
    if (T < 1 || T > RESAMP_MAX_TAPS) return 1;
    for (int phi = 0; phi < up && phi < T; ++phi) {
        long long sum = 0;
        for (int j = phi; j < T; j += up) {
            if (h[j] == -32768) return 2;
            sum += abs((int) h[j]);
        }
        if (sum > 65535) return 3;
    }
    return 0;
}

void resample_plan(int up, int down, const int16_t *h, int T, int na, ResamplePlan &p)
{
    const int U = up, D = down;
    p.U = U;
    p.D = D;
    p.T = T;
    p.NA = na;
    p.H = (T - 1 + U - 1) / U;
    p.groups.assign((size_t) U, ResampGroup{0, 0, 0});
    int base = 0;
    for (int i = 0; i < U; ++i) {
        const int first = floor_div(i * D - 1, U) + 1, next = floor_div((i + 1) * D - 1, U) + 1;
        p.groups[(size_t) i] = {first, next - first, base};
        base += (next - first + 1) / 2;
    }
    p.n_pairs = base;
    p.pairs.assign((size_t) base * (size_t) na, 0u);
    for (int i = 0; i < U; ++i) {
        const ResampGroup &g = p.groups[(size_t) i];
        auto tap = [&](int a, int r) -> int {        // sample r of the group, accumulator a
            if (r >= g.size) return 0;
            const int j = (i + a) * D + D - 1 - (g.first + r) * U;
            return (j >= 0 && j < T) ? h[j] : 0;
        };
        for (int q = 0; q < (g.size + 1) / 2; ++q)
            for (int a = 0; a < na; ++a)
                p.pairs[(size_t) (g.base + q) * (size_t) na + (size_t) a] =
                    (uint32_t) (uint16_t) tap(a, 2 * q) | ((uint32_t) (uint16_t) tap(a, 2 * q + 1) << 16);
    }
}

int resampler_fast_na(int K, int T, int D)
{
    if (K < 1 || K > 4) return 0;
    return (T + D - 1) / D <= RESAMP_FAST_NA ? RESAMP_FAST_NA : 0;
}

int channeliser_fast_na(int K, int T, int D)
{
    const int na = (T + D - 1) / D;
    if (K < 1 || K > 4) return 0;
    for (int b : {4, 8, 17}) if (na <= b) return b;
    if (na <= 33 && K <= 2) return 33;
    return 0;
}

} // namespace gnuais
