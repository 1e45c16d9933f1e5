// frame_time_kernel_main.cpp -- TEST INFRASTRUCTURE: frame_time.hip's own text on the CPU (tests/test_uptime_cpu.py builds
// it under ASan + UBSan with tests/c/hip_cpu in front of the HIP headers).  Every buffer has exactly the size the launch
// interface promises (kernels.h: FrameTimeLaunch): frames [frame_cap] records, frame_count [4], ctl [HDLC_CTL_WORDS][N],
// segcnt [N][n_seg], times [frame_cap].  launch_frame_times() runs every case; a case that names a grid runs on that grid
// as well, which makes the grid-stride loop turn, and must leave the same bytes.
// argv: in out.  in, case after case until the file ends: int64 N, n_seg, seg_words, len, n0, frame_cap, count, blocks
// (0: only what launch_frame_times() takes); then uint32 frames [frame_cap][16], uint32 ctl [6][N], uint32 segcnt
// [N][n_seg], int64 times [frame_cap] as they stand before the launch.  out, per case: int64 times [frame_cap] behind it.
#include <hip/hip_runtime.h>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "frame_time.hip"

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
        const uint32_t frame_cap = (uint32_t) hd[5];
        std::vector<uint32_t> frames((size_t) frame_cap * 16), count(4, 0), ctl((size_t) HDLC_CTL_WORDS * N);
        std::vector<uint32_t> segcnt((size_t) N * n_seg);
        std::vector<int64_t> times((size_t) frame_cap);
        if (fread(frames.data(), 4, frames.size(), f) != frames.size() || fread(ctl.data(), 4, ctl.size(), f) != ctl.size() ||
            fread(segcnt.data(), 4, segcnt.size(), f) != segcnt.size() || fread(times.data(), 8, times.size(), f) != times.size())
            return 4;
        count[0] = (uint32_t) hd[6];
        std::vector<int64_t> times_lib(times);
        FrameTimeLaunch a;
        a.frames = frames.data(); a.frame_count = count.data(); a.frame_cap = frame_cap; a.ctl = ctl.data();
        a.segcnt = segcnt.data(); a.times = times_lib.data(); a.N = N; a.n_seg = n_seg; a.seg_words = seg_words;
        a.len = len; a.n0 = hd[4];
        if (launch_frame_times(a, nullptr) != hipSuccess) return 6;
        if (hd[7]) {
            hipLaunchKernelGGL(frame_time_kernel, dim3((unsigned) hd[7]), dim3(FT_BLOCK), 0, nullptr, (const uint32_t *) a.frames,
                               a.frame_count, a.frame_cap, a.ctl, a.segcnt, (long long *) times.data(), a.N, a.n_seg,
                               a.seg_words * 32, a.len, (long long) a.n0);
            if (times != times_lib) return 7;
        }
        fwrite(times_lib.data(), 8, times_lib.size(), g);
        ++n_cases;
    }
    fclose(f);
    fclose(g);
    printf("cases: %d\n", n_cases);
    return 0;
}
