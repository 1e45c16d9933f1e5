// Issue rate of v_dot2c_i32_i16 (__builtin_amdgcn_sdot2 on short2) on gfx950: 8 independent accumulators per lane, a
// long unrolled chain, 8 workgroups of 256 per CU.  -> lane instructions per second (against 256 x 4 x 16 x 2.4e9 = 3.9e13).
// (channeliser.hip: the tap sum of the fast form is these instructions.)
#include <hip/hip_runtime.h>
#include <cstdio>
typedef short short2_t __attribute__((ext_vector_type(2)));
constexpr int ITERS = 4096, UNR = 16, ACC = 8;

__global__ __launch_bounds__(256) void k_dot2(int *out, unsigned a0, unsigned b0)
{
    int acc[ACC];
    unsigned a = a0 ^ threadIdx.x, b = b0;
    for (int j = 0; j < ACC; ++j) acc[j] = j;
    for (int i = 0; i < ITERS; ++i)
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int j = 0; j < ACC; ++j)
                acc[j] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, a), __builtin_bit_cast(short2_t, b), acc[j], false);
    int s = 0;
    for (int j = 0; j < ACC; ++j) s += acc[j];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

int main()
{
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    const int blocks = p.multiProcessorCount * 8, threads = blocks * 256;
    int *o;
    hipMalloc(&o, sizeof(int) * threads);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const double ops = (double) threads * ITERS * UNR * ACC;
    {
        float best = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            hipEventRecord(e0);
            hipLaunchKernelGGL(k_dot2, dim3(blocks), dim3(256), 0, 0, o, 0x00030005u, 0x00070002u);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (rep && ms < best) best = ms;
        }
        printf("{\"op\": \"%s\", \"cus\": %d, \"ms\": %.4f, \"lane_ops_per_s\": %.4g}\n",
               "v_dot2c_i32_i16", p.multiProcessorCount, best, ops / (best * 1e-3));
    }
    hipFree(o);
    return 0;
}
