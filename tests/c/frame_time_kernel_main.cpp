// frame_time_kernel_main.cpp -- TEST INFRASTRUCTURE: frame_time.hip's kernel, its own text, on the CPU
// (tests/test_uptime_cpu.py builds it under ASan + UBSan with tests/c/hip_grid_shim in front of the HIP headers): a
// std::thread per lane, one block at a time.  Every buffer has exactly the size the launch interface promises
// (kernels.h: FrameTimeLaunch): frames [frame_cap] records, frame_count [4], ctl [HDLC_CTL_WORDS][N], segcnt [N][n_seg],
// times [frame_cap].
// argv: in out.  in, case after case until the file ends: int64 N, n_seg, seg_words, len, n0, frame_cap, count, blocks
// (0: what launch_frame_times() takes); then uint32 frames [frame_cap][16], uint32 ctl [6][N], uint32 segcnt [N][n_seg],
// int64 times [frame_cap] as they stand before the launch.  out, per case: int64 times [frame_cap] behind it.
#include <hip/hip_runtime.h>
#include <thread>
#include <vector>
#include <functional>
#include <cstdio>
#include <cstdlib>
thread_local Idx threadIdx;
Idx blockIdx, gridDim;
std::barrier<> *g_block_barrier;
std::barrier<> *g_wave_barrier[4];
unsigned char g_pred[256];
#include "frame_time.hip"

// `blocks` blocks of 256 threads, one block at a time
static void run_grid(unsigned blocks, const std::function<void()> &kernel)
{
    gridDim.x = blocks;
    for (unsigned b = 0; b < blocks; ++b) {
        blockIdx.x = b;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < 256; ++t)
            th.emplace_back([&, t] {
                threadIdx.x = t;
                kernel();
            });
        for (auto &t : th) t.join();
    }
}

int main(int argc, char **argv)
{
    using namespace gnuais;
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    int64_t hd[8];
    int n_cases = 0;
    while (fread(hd, 8, 8, f) == 8) {
        const int N = (int) hd[0], n_seg = (int) hd[1], seg_words = (int) hd[2], len = (int) hd[3];
        const long long n0 = hd[4];
        const uint32_t frame_cap = (uint32_t) hd[5];
        std::vector<uint32_t> frames((size_t) frame_cap * 16), count(4, 0), ctl((size_t) HDLC_CTL_WORDS * N);
        std::vector<uint32_t> segcnt((size_t) N * n_seg);
        std::vector<long long> times((size_t) frame_cap);
        if (fread(frames.data(), 4, frames.size(), f) != frames.size() || fread(ctl.data(), 4, ctl.size(), f) != ctl.size() ||
            fread(segcnt.data(), 4, segcnt.size(), f) != segcnt.size() || fread(times.data(), 8, times.size(), f) != times.size())
            return 4;
        count[0] = (uint32_t) hd[6];
        const unsigned want = (frame_cap + FT_BLOCK - 1) / FT_BLOCK;
        const unsigned blocks = hd[7] ? (unsigned) hd[7] : want < 1u ? 1u : want > (unsigned) FT_MAX_BLOCKS ? (unsigned) FT_MAX_BLOCKS : want;
        run_grid(blocks, [&] {
            frame_time_kernel(frames.data(), count.data(), frame_cap, ctl.data(), segcnt.data(), times.data(), N, n_seg,
                              seg_words * 32, len, n0);
        });
        fwrite(times.data(), 8, times.size(), g);
        ++n_cases;
    }
    fclose(f);
    fclose(g);
    printf("cases: %d\n", n_cases);
    return 0;
}
