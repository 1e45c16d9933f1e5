// wide_launch.hip -- the one launch of the wide stage (kernels.h: launch_wide): the argument checks, the segments, the
// choice of the form and the carry copy, for every ratio and sample format.  Host code only; the kernels are
// wide_kernels.h, instantiated by channeliser.hip, channeliser_fmt.hip and resampler.hip.
#include <algorithm>

#include "kernels.h"
#include "wide_format.h"

namespace gnuais {
namespace {

template <int F>
hipError_t launch_wide_f(const WideLaunch &a, long long blocks, uint32_t *hist_out, hipStream_t stream)
{
    if (a.NA > 0) {
        const dim3 grid((unsigned) blocks);
        // the group table makes the ratio a rational one; without it the groups are the integer form's
        const hipError_t e = a.groups ? wide_fast_launch<F, true>(a, grid, stream) : wide_fast_launch<F, false>(a, grid, stream);
        if (e != hipSuccess) return e;
    } else {
        wide_direct_launch<F>(a, dim3((unsigned) blocks, (unsigned) a.K), stream);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.H > 0) wide_carry_launch<F>(a, hist_out, stream);
    return hipGetLastError();
}

} // namespace

hipError_t launch_wide(const WideLaunch &a0, int fmt, uint32_t *hist_out, hipStream_t stream)
{
    WideLaunch a = a0;
    if (a.M <= 0 || a.K <= 0 || a.K > CHAN_MAX_K || a.U < 1 || (a.U == 1 ? a.D < 1 : a.D <= a.U) || a.len <= 0 ||
        a.len % a.D || a.T < 1 || a.H != (a.T - 1 + a.U - 1) / a.U)
        return hipErrorInvalidValue;
    const long long rows = (long long) (a.len / a.D) * a.U;
    if (rows > 0x7fffffffLL) return hipErrorInvalidValue;
    a.n_groups = (a.M + 63) / 64;
    // segments: enough waves to fill the chip (about 4096), no shorter than 128 rows (the halo is NA-1 groups)
    const long long want = (rows * a.n_groups + 4095) / 4096;
    a.seg_rows = (int) std::min<long long>(2048, std::max<long long>(128, want));
    const long long n_seg = (rows + a.seg_rows - 1) / a.seg_rows;
    const long long blocks = n_seg * a.n_groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    switch (fmt) {
    case FMT_CS16: return launch_wide_f<FMT_CS16>(a, blocks, hist_out, stream);
    case FMT_CU8: return launch_wide_f<FMT_CU8>(a, blocks, hist_out, stream);
    case FMT_CS8: return launch_wide_f<FMT_CS8>(a, blocks, hist_out, stream);
    case FMT_CF32: return launch_wide_f<FMT_CF32>(a, blocks, hist_out, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gnuais
