// TEST INFRASTRUCTURE: rocprim::radix_sort_pairs' interface on the CPU (tests/c/hip_cpu): a size query with a
// null temporary, then a STABLE sort on bits [begin_bit, end_bit) of the keys, into the output arrays
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
namespace rocprim {
template <class K, class V>
inline hipError_t radix_sort_pairs(void *tmp, size_t &bytes, const K *kin, K *kout, const V *vin, V *vout, size_t n,
                                   unsigned begin_bit, unsigned end_bit, hipStream_t)
{
    if (!tmp) { bytes = 256; return hipSuccess; }
    if (kin == kout || vin == vout || end_bit <= begin_bit || end_bit > 8 * sizeof(K)) return hipErrorInvalidValue;
    const K mask = end_bit - begin_bit >= 8 * sizeof(K) ? ~K(0) : ((K(1) << (end_bit - begin_bit)) - 1);
    std::vector<size_t> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = i;
    std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) { return ((kin[a] >> begin_bit) & mask) < ((kin[b] >> begin_bit) & mask); });
    for (size_t i = 0; i < n; ++i) { kout[i] = kin[o[i]]; vout[i] = vin[o[i]]; }
    return hipSuccess;
}
}
