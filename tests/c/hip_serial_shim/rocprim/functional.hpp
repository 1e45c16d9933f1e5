// TEST INFRASTRUCTURE: rocprim::plus for the CPU build of frame_unique.hip (tests/c/hip_serial_shim)
#pragma once
namespace rocprim { template <class T> struct plus { T operator()(T a, T b) const { return a + b; } }; }
