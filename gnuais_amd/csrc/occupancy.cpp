// occupancy.cpp -- gnuais_occupancy_code, _power and _cover_span (include/gnuais_hip.h): the arithmetic of occupancy.h as
// host entries, the text the kernels of occupancy.hip run.  Plain C++, no HIP (tests/test_occupancy_cpu.py runs it on the
// CPU).
#include "occupancy.h"

#include "../../include/gnuais_hip.h"

extern "C" int gnuais_occupancy_code(long long P, int *code)
{
    if (!code || P < 0 || P >= (1LL << 38)) return GNUAIS_E_ARG;
    *code = gnuais::occ_code(P);
    return GNUAIS_OK;
}

extern "C" int gnuais_occupancy_power(int code, long long *P)
{
    if (!P || code < 0 || code > gnuais::OCC_BINS) return GNUAIS_E_ARG;      // 288: the upper edge of the last bin
    *P = gnuais::occ_power(code);
    return GNUAIS_OK;
}

extern "C" int gnuais_occupancy_cover_span(long long t, int nbits, unsigned pllinc, int n_taps, int afc_window, long long v0,
                                           long long *j_lo, int *nb)
{
    if (!j_lo || !nb || nbits < 0 || nbits > 0xffff || pllinc == 0 || pllinc > 0xffffu || n_taps < 0 || afc_window < 0)
        return GNUAIS_E_ARG;
    (void) gnuais::occ_cover_span(t, nbits, pllinc, n_taps, afc_window, v0, j_lo, nb);
    return GNUAIS_OK;
}
