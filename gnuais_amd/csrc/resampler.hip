// resampler.hip -- the wide stage's fast form at a rational ratio U/D (gnuais_batch_resampler, include/gnuais_hip.h), for
// captures whose rate is no integer multiple of the chain's: channeliser_kernel<K, 17, F, true> of wide_kernels.h for K = 1..4 and
// every sample format.  Its direct form and carry copy are the integer ratio's (channeliser.hip, channeliser_fmt.hip).
#include "wide_kernels.h"

namespace gnuais {

template hipError_t wide_fast_launch<FMT_CS16, true>(const WideLaunch &, dim3, hipStream_t);
template hipError_t wide_fast_launch<FMT_CU8, true>(const WideLaunch &, dim3, hipStream_t);
template hipError_t wide_fast_launch<FMT_CS8, true>(const WideLaunch &, dim3, hipStream_t);
template hipError_t wide_fast_launch<FMT_CF32, true>(const WideLaunch &, dim3, hipStream_t);

} // namespace gnuais
