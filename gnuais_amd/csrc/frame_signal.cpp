// frame_signal.cpp -- gnuais_frame_signal_span (include/gnuais_hip.h): the span arithmetic of frame_signal.h as a host
// entry, the text frame_signal_kernel runs.  Plain C++, no HIP (tests/test_frame_signal_cpu.py runs it on the CPU).
#include "frame_signal.h"

#include "../../include/gnuais_hip.h"

extern "C" int gnuais_frame_signal_span(long long t, int nbits, unsigned pllinc, int n_taps, int afc_window, long long v0,
                                        long long *j_lo, int *nb)
{
    if (!j_lo || !nb || nbits < 0 || nbits > 0xffff || pllinc == 0 || pllinc > 0xffffu || n_taps < 0 || afc_window < 0)
        return GNUAIS_E_ARG;
    (void) gnuais::fs_span(t, nbits, pllinc, n_taps, afc_window, v0, j_lo, nb);
    return GNUAIS_OK;
}
