// channeliser.hip -- the wide stage's kernels (wide_kernels.h) on int16 wide samples (GNUAIS_FMT_CS16): the fast form at an
// integer ratio, the direct form and the carry copy.  The other formats' are in channeliser_fmt.hip, the fast form at a
// rational ratio in resampler.hip.
#include "wide_kernels.h"

namespace gnuais {

template hipError_t wide_fast_launch<FMT_CS16, false>(const WideLaunch &, dim3, hipStream_t);
template void wide_direct_launch<FMT_CS16>(const WideLaunch &, dim3, hipStream_t);
template void wide_carry_launch<FMT_CS16>(const WideLaunch &, uint32_t *, hipStream_t);

} // namespace gnuais
