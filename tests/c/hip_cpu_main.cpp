// hip_cpu_main.cpp -- TEST INFRASTRUCTURE: tests/c/hip_cpu itself, which every CPU kernel program rests on
// (tests/test_hip_cpu_shim.py builds this under ASan + UBSan).  A host program: nothing here touches a device.
//   argv: grid          3 blocks x 128 lanes, then 1 block x 100 lanes: per lane blockIdx, threadIdx, its wave's ballot of
//                       threadIdx % 3 == 0, the word the block's last lane put into static __shared__ in front of a
//                       barrier, gridDim, blockDim -- printed one lane per line
//   argv: lds <reach>   2 blocks x 64 lanes with 100 bytes of dynamic shared memory: every block counts the bytes that
//                       already hold the pattern the lanes then write, and lane 0 reads byte reach - 1.  Prints the counts.
//   argv: early         1 block x 128 lanes: the odd lanes return at once, the even ones meet at a barrier and vote
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

HIP_DYNAMIC_SHARED(unsigned char, lds_bytes)        // at namespace scope; lds_kernel has one of its own as well
constexpr unsigned LDS_BYTES = 100;
constexpr unsigned char PATTERN = 0x5c;

__global__ void grid_kernel(unsigned long long *out)
{
    __shared__ uint32_t word;
    if (threadIdx.x == blockDim.x - 1) word = 1000 + blockIdx.x;
    __syncthreads();
    const unsigned long long vote = __ballot(threadIdx.x % 3 == 0);
    unsigned long long *o = out + ((size_t) blockIdx.x * blockDim.x + threadIdx.x) * 6;
    o[0] = blockIdx.x; o[1] = threadIdx.x; o[2] = vote; o[3] = word; o[4] = gridDim.x; o[5] = blockDim.x;
}

__global__ void lds_kernel(unsigned reach, uint32_t *stale, uint32_t *misaligned, volatile unsigned char *sink)
{
    HIP_DYNAMIC_SHARED(unsigned char, mine)
    unsigned char *p = mine;
    if (threadIdx.x == 0 && (p != lds_bytes || (uintptr_t) p % 16)) *misaligned = 1;
    for (unsigned i = threadIdx.x; i < LDS_BYTES; i += blockDim.x)
        if (mine[i] == PATTERN) atomicAdd(&stale[blockIdx.x], 1u);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < LDS_BYTES; i += blockDim.x) lds_bytes[i] = PATTERN;
    __syncthreads();
    if (threadIdx.x == 0) *sink = mine[reach - 1];
}

__global__ void early_kernel(unsigned long long *out)
{
    out[threadIdx.x] = 1;
    if (threadIdx.x & 1) return;
    __syncthreads();
    out[threadIdx.x] = __ballot(true);
}

static void print_lanes(const std::vector<unsigned long long> &out)
{
    for (size_t i = 0; i < out.size(); i += 6)
        printf("%llu %llu %llx %llu %llu %llu\n", out[i], out[i + 1], out[i + 2], out[i + 3], out[i + 4], out[i + 5]);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "grid")) {
        std::vector<unsigned long long> a((size_t) 3 * 128 * 6, 77), b((size_t) 100 * 6, 77);
        hipLaunchKernelGGL(grid_kernel, dim3(3), dim3(128), 0, nullptr, a.data());
        hipLaunchKernelGGL(grid_kernel, dim3(1), dim3(100), 0, nullptr, b.data());
        print_lanes(a);
        print_lanes(b);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "lds")) {
        uint32_t stale[2] = {0, 0}, misaligned = 0;
        unsigned char sink = 0;
        hipLaunchKernelGGL(lds_kernel, dim3(2), dim3(64), LDS_BYTES, nullptr, (unsigned) atoi(argv[2]), stale, &misaligned, &sink);
        printf("%u %u %u %u\n", stale[0], stale[1], misaligned, (unsigned) sink);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "early")) {
        std::vector<unsigned long long> out(128, 77);
        hipLaunchKernelGGL(early_kernel, dim3(1), dim3(128), 0, nullptr, out.data());
        for (unsigned long long v : out) printf("%llx\n", v);
        return 0;
    }
    return 2;
}
