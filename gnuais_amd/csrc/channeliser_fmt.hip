// channeliser_fmt.hip -- the kernels of channeliser.hip on wide samples that are not int16: unsigned and signed 8-bit pairs
// and fp32 pairs, as SDRs write them (GNUAIS_FMT_CU8 / _CS8 / _CF32, defined in include/gnuais_hip.h), converted where a
// lane loads its sample (wide_kernels.h).  Every (K, NA) instance of the integer fast form, the direct form and the carry
// copy exist once per format.
#include "wide_kernels.h"

namespace gnuais {

template hipError_t wide_fast_launch<FMT_CU8, false>(const WideLaunch &, dim3, hipStream_t);
template hipError_t wide_fast_launch<FMT_CS8, false>(const WideLaunch &, dim3, hipStream_t);
template hipError_t wide_fast_launch<FMT_CF32, false>(const WideLaunch &, dim3, hipStream_t);
template void wide_direct_launch<FMT_CU8>(const WideLaunch &, dim3, hipStream_t);
template void wide_direct_launch<FMT_CS8>(const WideLaunch &, dim3, hipStream_t);
template void wide_direct_launch<FMT_CF32>(const WideLaunch &, dim3, hipStream_t);
template void wide_carry_launch<FMT_CU8>(const WideLaunch &, uint32_t *, hipStream_t);
template void wide_carry_launch<FMT_CS8>(const WideLaunch &, uint32_t *, hipStream_t);
template void wide_carry_launch<FMT_CF32>(const WideLaunch &, uint32_t *, hipStream_t);

} // namespace gnuais
