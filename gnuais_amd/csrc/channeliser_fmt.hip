// channeliser_fmt.hip -- the channeliser (channeliser.hip) on wide samples that are not int16: unsigned and signed 8-bit
// pairs and fp32 pairs, as SDRs write them (GNUAIS_FMT_CU8 / _CS8 / _CF32, defined in include/gnuais_hip.h).  The same
// text as the int16 kernels (channeliser_kernels.inc over channeliser_body.h) with the conversion where a lane loads its wide sample -- 2 bytes per
// lane for the 8-bit formats, 8 for cf32 -- so no int16 copy of the wide stream is ever written.  Every (K, NA) instance of
// the fast form, the direct form and the carry copy exist once per format; the carry holds converted int16 words, so
// calls of different formats may follow each other on one batch.
#include "channeliser_body.h"

namespace gnuais {

#define CHAN_FAST_TEMPLATE template <int K, int NA, int F>
#define CHAN_FMT_TEMPLATE template <int F>
#define CHAN_FAST_KERNEL channeliser_fmt_kernel
#define CHAN_DIRECT_KERNEL channeliser_fmt_direct_kernel
#define CHAN_CARRY_KERNEL channeliser_fmt_carry_kernel
#define CHAN_F F
#include "channeliser_kernels.inc"

namespace {
template <int F>
struct FmtKernels {
    template <int K, int NA>
    static void fast(const ChanLaunch &a, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((channeliser_fmt_kernel<K, NA, F>), grid, dim3(64), 0, stream, a);
    }
    static void direct(const ChanLaunch &a, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL(channeliser_fmt_direct_kernel<F>, grid, dim3(64), 0, stream, a);
    }
    static void carry(dim3 grid, hipStream_t stream, const void *in, const uint32_t *hist_in, uint32_t *hist_out, int M,
                      int T, int len)
    {
        hipLaunchKernelGGL(channeliser_fmt_carry_kernel<F>, grid, dim3(256), 0, stream, in, hist_in, hist_out, M, T, len);
    }
};
} // namespace

hipError_t launch_channeliser_fmt(const ChanLaunch &a, int fmt, uint32_t *hist_out, hipStream_t stream)
{
    switch (fmt) {
    case FMT_CU8: return launch_chan_with<FmtKernels<FMT_CU8>>(a, hist_out, stream);
    case FMT_CS8: return launch_chan_with<FmtKernels<FMT_CS8>>(a, hist_out, stream);
    case FMT_CF32: return launch_chan_with<FmtKernels<FMT_CF32>>(a, hist_out, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gnuais
