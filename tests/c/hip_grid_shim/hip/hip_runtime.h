// hip_grid_shim/hip/hip_runtime.h -- TEST INFRASTRUCTURE: tests/c/hip_block_shim's names and gridDim, which a grid-stride
// kernel reads (tests/c/occupancy_kernel_main.cpp sets it before it runs a kernel's blocks one at a time).
#pragma once
#include "../../hip_block_shim/hip/hip_runtime.h"
extern Idx gridDim;
