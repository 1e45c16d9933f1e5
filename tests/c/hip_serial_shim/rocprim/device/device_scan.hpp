// TEST INFRASTRUCTURE: rocprim::inclusive_scan's interface on the CPU (tests/c/hip_serial_shim): a size query with a
// null temporary, then the scan
#pragma once
#include <hip/hip_runtime.h>
namespace rocprim {
template <class T, class Op>
inline hipError_t inclusive_scan(void *tmp, size_t &bytes, const T *in, T *out, size_t n, Op op, hipStream_t)
{
    if (!tmp) { bytes = 256; return hipSuccess; }
    T acc = T();
    for (size_t i = 0; i < n; ++i) out[i] = acc = i ? op(acc, in[i]) : in[i];
    return hipSuccess;
}
}
