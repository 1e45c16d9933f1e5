// channeliser.hip -- wideband in: tune, low-pass and decimate int16 (I, Q) streams into the narrowband I/Q the
// discriminator takes (gnuais_batch_run_wideband, include/gnuais_hip.h).  Not part of the reference; all integer, defined
// exactly in the header and restated in NumPy (tests/chan_ref.py), so the device matches it bit for bit whatever the
// order of the sums.
//
// Layout: in [len][M] words (I lo, Q hi), out [len/D][M*K] words, receiver c = s*K + k.  A lane owns one stream and all
// K offsets: it reads each wide sample once, mixes it for every offset, and walks a segment of output rows.  The mixer
// row and the taps depend on the time index alone, which is the same in every lane of a workgroup (lanes are streams,
// the segment is the workgroup's), so they are uniform loads.  Results leave with vector stores only.
//
// Fast form (channeliser_kernel<K, NA>): transposed polyphase.  With wide sample i = g*D + r of group g, output m = g + a
// takes it with tap j = a*D + D-1-r, so each mixed sample feeds the NA = ceil(T/D) outputs g .. g+NA-1, whose int32
// accumulators live in registers; after group g, output g is complete, leaves, and the accumulators shift by one.  Two
// consecutive samples of a group go into one v_dot2c_i32_i16 per accumulator (__builtin_amdgcn_sdot2): the taps are
// pre-packed on the host as pairs (h[aD + D-1-r], h[aD + D-2-r]) = POLY[r/2][a], zero where a tap index is >= T or the
// group has an odd last sample.  A segment starts NA-1 groups early to fill its accumulators (the halo: (NA-1)*D wide
// samples, ~1 % of a 1500-row segment); samples before the call come from the carry, before that they are zero.
//
// Direct form (channeliser_direct_kernel): any K and T, one lane per (stream, offset), every tap mixes its sample again.
// Used only where the fast form's accumulators do not fit in registers (K > 4, or ceil(T/D) above the largest bucket):
// filters far longer than the default 16 D + 1 taps.
//
// The carry (the last T-1 wide samples per stream) is double-buffered: a launch reads one buffer and
// channeliser_carry_kernel writes the other, so no launch reads what it writes.
//
// The text of all three kernels is channeliser_kernels.inc over channeliser_body.h, with the input's sample format as a
// parameter; the kernels here are the int16 (GNUAIS_FMT_CS16) ones, channeliser_fmt.hip holds those of the other formats.
#include "channeliser_body.h"

namespace gnuais {

#define CHAN_FAST_TEMPLATE template <int K, int NA>
#define CHAN_FMT_TEMPLATE
#define CHAN_FAST_KERNEL channeliser_kernel
#define CHAN_DIRECT_KERNEL channeliser_direct_kernel
#define CHAN_CARRY_KERNEL channeliser_carry_kernel
#define CHAN_F FMT_CS16
#include "channeliser_kernels.inc"

int channeliser_fast_na(int K, int T, int D)
{
    const int na = (T + D - 1) / D;
    if (K < 1 || K > 4) return 0;
    for (int b : {4, 8, 17}) if (na <= b) return b;
    if (na <= 33 && K <= 2) return 33;
    return 0;
}

namespace {
struct Cs16Kernels {
    template <int K, int NA>
    static void fast(const ChanLaunch &a, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((channeliser_kernel<K, NA>), grid, dim3(64), 0, stream, a);
    }
    static void direct(const ChanLaunch &a, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL(channeliser_direct_kernel, grid, dim3(64), 0, stream, a);
    }
    static void carry(dim3 grid, hipStream_t stream, const void *in, const uint32_t *hist_in, uint32_t *hist_out, int M,
                      int T, int len)
    {
        hipLaunchKernelGGL(channeliser_carry_kernel, grid, dim3(256), 0, stream, in, hist_in, hist_out, M, T, len);
    }
};
} // namespace

hipError_t launch_channeliser(const ChanLaunch &a, int fmt, uint32_t *hist_out, hipStream_t stream)
{
    if (fmt == FMT_CS16) return launch_chan_with<Cs16Kernels>(a, hist_out, stream);
    return launch_channeliser_fmt(a, fmt, hist_out, stream);
}

} // namespace gnuais
