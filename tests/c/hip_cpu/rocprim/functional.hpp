// TEST INFRASTRUCTURE: rocprim::plus for the CPU builds of the kernel files (tests/c/hip_cpu)
#pragma once
namespace rocprim { template <class T> struct plus { T operator()(T a, T b) const { return a + b; } }; }
