// repair_kernel_main.cpp -- TEST INFRASTRUCTURE: hdlc_repair.hip's own text on the CPU, run through launch_hdlc_repair()
// (tests/test_repair_cpu.py builds it under ASan + UBSan with tests/c/hip_cpu in front of the HIP headers).
// argv: in out.  in: int32 N, K, frame_cap; cand [N][K][20] u32; cand_first [N]; cand_count [N].
// out: the ring's four counters, repaired [N], the ring's records.
#include <hip/hip_runtime.h>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "hdlc_repair.hip"
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
    gnuais::RepairLaunch a;
    a.cand = cand.data(); a.cand_first = first.data(); a.cand_count = count.data(); a.repaired = repaired.data();
    a.frames = frames.data(); a.frame_count = flags; a.frame_cap = (uint32_t) cap; a.N = N; a.K = K;
    if (gnuais::launch_hdlc_repair(a, nullptr) != hipSuccess) return 4;
    FILE *g = fopen(argv[2], "wb");
    fwrite(flags, 4, 4, g);
    fwrite(repaired.data(), 4, N, g);
    const uint32_t have = flags[0] < (uint32_t) cap ? flags[0] : (uint32_t) cap;
    fwrite(frames.data(), 64, have, g);
    fclose(g);
    return 0;
}
