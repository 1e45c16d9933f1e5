// repair_kernel_main.cpp -- TEST INFRASTRUCTURE: hdlc_repair_kernel's own text on the CPU (tests/test_repair_cpu.py builds
// it under ASan + UBSan with tests/c/hip_block_shim in front of the HIP headers): a std::thread per lane, one block at a
// time.  REPAIR_KERNEL_TEXT is a copy of hdlc_repair.hip whose dynamic shared array is an ordinary declaration.
// argv: in out.  in: int32 N, K, frame_cap; cand [N][K][20] u32; cand_first [N]; cand_count [N].
// out: the ring's four counters, repaired [N], the ring's records.
#include <hip/hip_runtime.h>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdlib>
thread_local Idx threadIdx;
Idx blockIdx;
std::barrier<> *g_block_barrier;
std::barrier<> *g_wave_barrier[4];
unsigned char g_pred[256];
namespace gnuais { namespace { uint32_t rp_rows[256 * 21]; } }
#include REPAIR_KERNEL_TEXT
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int32_t N, K, cap;
    if (fread(&N, 4, 1, f) != 1 || fread(&K, 4, 1, f) != 1 || fread(&cap, 4, 1, f) != 1) return 2;
    std::vector<uint32_t> cand((size_t) N * K * 20), first(N), count(N), frames((size_t) cap * 16, 0xdeadbeef);
    if (fread(cand.data(), 4, cand.size(), f) != cand.size() || fread(first.data(), 4, N, f) != (size_t) N ||
        fread(count.data(), 4, N, f) != (size_t) N) return 3;
    fclose(f);
    std::vector<int32_t> repaired(N, 0);
    uint32_t flags[4] = {0, 0, 0, 0};
    const int blocks = (N + 31) / 32;
    for (int b = 0; b < blocks; ++b) {
        blockIdx.x = b;
        std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
        g_block_barrier = &bb;
        g_wave_barrier[0] = &w0; g_wave_barrier[1] = &w1; g_wave_barrier[2] = &w2; g_wave_barrier[3] = &w3;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < 256; ++t)
            th.emplace_back([&, t] {
                threadIdx.x = t;
                gnuais::hdlc_repair_kernel(cand.data(), first.data(), count.data(), repaired.data(), frames.data(), flags,
                                           (uint32_t) cap, N, K);
            });
        for (auto &t : th) t.join();
    }
    FILE *g = fopen(argv[2], "wb");
    fwrite(flags, 4, 4, g);
    fwrite(repaired.data(), 4, N, g);
    const uint32_t have = flags[0] < (uint32_t) cap ? flags[0] : (uint32_t) cap;
    fwrite(frames.data(), 64, have, g);
    fclose(g);
    return 0;
}
