// TEST INFRASTRUCTURE: rocprim's two scans on the CPU (tests/c/hip_cpu): a size query with a null temporary, then the scan
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
template <class T, class Op>
inline hipError_t exclusive_scan(void *tmp, size_t &bytes, const T *in, T *out, T init, size_t n, Op op, hipStream_t)
{
    if (!tmp) { bytes = 256; return hipSuccess; }
    T acc = init;
    for (size_t i = 0; i < n; ++i) { const T v = in[i]; out[i] = acc; acc = op(acc, v); }
    return hipSuccess;
}
}
