// long_kernel_main.cpp -- TEST INFRASTRUCTURE: hdlc_long.hip's own text on the CPU, run through launch_hdlc_long_reset()
// and launch_hdlc_long() (tests/test_long_cpu.py builds it under ASan + UBSan with tests/c/hip_cpu in front of the HIP
// headers).  Every buffer has exactly the size the launch interface promises (kernels.h: LongLaunch).  The chain's
// deframer, whose bit count D' reads, is stood in for by its count alone: ctl[2] / ctl[5] move on by the bits of a call's
// packs before the kernel runs, as they have when the launch behind K3 starts.
// argv: in out.  in: int64 N, n_seg, seg_words, frame_cap, n_calls; uint64 bits fed before the first call [N]; then per
// call int64 len, n0, uint32 segbits [N][n_seg][16], uint32 segcnt [N][n_seg].
// out: per call uint32 lctl [3][N]; then int32 counters [2][N], uint32 frame_count [2], the ring's records.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "hdlc_long.hip"

int main(int argc, char **argv)
{
    using namespace gnuais;
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    int64_t hd[5];
    if (fread(hd, 8, 5, f) != 5) return 3;
    const int N = (int) hd[0], n_seg = (int) hd[1], seg_words = (int) hd[2];
    const uint32_t cap = (uint32_t) hd[3];
    const int n_calls = (int) hd[4];
    std::vector<uint64_t> seen(N);
    if (fread(seen.data(), 8, N, f) != (size_t) N) return 4;
    std::vector<uint32_t> ctl((size_t) HDLC_CTL_WORDS * N, 0), lctl((size_t) LONG_CTL_WORDS * N, 0xdeadbeefu);
    std::vector<uint32_t> open((size_t) LONG_REC_WORDS * N, 0xdeadbeefu), frames((size_t) cap * LONG_FRAME_WORDS, 0xdeadbeefu);
    std::vector<int32_t> counters((size_t) 2 * N, 0);
    uint32_t count[2] = {0, 0};
    if (launch_hdlc_long_reset(lctl.data(), nullptr, N, nullptr) != hipSuccess) return 8;
    for (int call = 0; call < n_calls; ++call) {
        int64_t lh[2];
        if (fread(lh, 8, 2, f) != 2) return 6;
        std::vector<uint32_t> segbits((size_t) N * n_seg * PACK_STRIDE), segcnt((size_t) N * n_seg);
        if (fread(segbits.data(), 4, segbits.size(), f) != segbits.size() || fread(segcnt.data(), 4, segcnt.size(), f) != segcnt.size())
            return 7;
        for (int c = 0; c < N; ++c) {
            for (int s = 0; s < n_seg; ++s) seen[c] += std::min<uint32_t>(segcnt[(size_t) c * n_seg + s], (uint32_t) seg_words * 32);
            ctl[(size_t) 2 * N + c] = (uint32_t) seen[c];
            ctl[(size_t) 5 * N + c] = (uint32_t) (seen[c] >> 32);
        }
        LongLaunch a;
        a.segbits = segbits.data(); a.segcnt = segcnt.data(); a.ctl = ctl.data(); a.lctl = lctl.data(); a.open = open.data();
        a.counters = counters.data(); a.frames = frames.data(); a.frame_count = count; a.frame_cap = cap;
        a.N = N; a.n_seg = n_seg; a.seg_words = seg_words; a.len = (int) lh[0]; a.n0 = lh[1];
        if (launch_hdlc_long(a, nullptr) != hipSuccess) return 9;
        fwrite(lctl.data(), 4, lctl.size(), g);
    }
    fwrite(counters.data(), 4, counters.size(), g);
    fwrite(count, 4, 2, g);
    fwrite(frames.data(), 4 * LONG_FRAME_WORDS, count[0] < cap ? count[0] : cap, g);
    fclose(f);
    fclose(g);
    return 0;
}
