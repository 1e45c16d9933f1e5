// TEST INFRASTRUCTURE: rocprim's two scans on the CPU (tests/c/hip_launch_shim): the inclusive one is hip_serial_shim's,
// the exclusive one -- a size query with a null temporary, then the scan -- is added here
#pragma once
#include "../../../hip_serial_shim/rocprim/device/device_scan.hpp"
namespace rocprim {
template <class T, class Op>
inline hipError_t exclusive_scan(void *tmp, size_t &bytes, const T *in, T *out, T init, size_t n, Op op, hipStream_t)
{
    if (!tmp) { bytes = 256; return hipSuccess; }
    T acc = init;
    for (size_t i = 0; i < n; ++i) { const T v = in[i]; out[i] = acc; acc = op(acc, v); }
    return hipSuccess;
}
}
