// long_repair_kernel_main.cpp -- TEST INFRASTRUCTURE: hdlc_long.hip's kernel in its form that keeps the raw bits and
// hdlc_long_repair.hip's kernel, their own text, on the CPU (tests/test_long_repair_cpu.py builds it under ASan + UBSan
// with tests/c/hip_wave_shim in front of the HIP headers): a std::thread per lane, one block of 64 at a time.  Every
// buffer has exactly the size the launch interface promises (kernels.h: LongLaunch, LongRepairLaunch).  Per call: the
// chain's deframer's count moves on (as in long_kernel_main.cpp), D' runs over the packs, then the repair over what D'
// listed, on `blocks` workgroups; the two candidate counters are used by call parity as the library uses them.
// argv: in out.  in: int64 N, n_seg, seg_words, frame_cap, n_calls, cand_cap, blocks; uint64 bits fed before the first
// call [N]; then per call int64 len, n0, uint32 segbits [N][n_seg][16], uint32 segcnt [N][n_seg].
// out: per call uint32 lctl [3][N], uint32 candidates listed; then int32 counters [3][N], uint32 frame_count [2], the
// ring's records.
#include <hip/hip_runtime.h>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdlib>
thread_local Idx threadIdx;
Idx blockIdx, blockDim;
std::barrier<> *g_block_barrier;
std::barrier<> *g_wave_barrier[4];
unsigned char g_pred[256];
namespace gnuais { uint32_t long_pack[(16 + 1) * 64]; }
#include "hdlc_long.hip"
#undef __shared__
#define __shared__ static       // the repair kernel's arrays are static shared memory: one per block, one block at a time
#include "hdlc_long_repair.hip"

template <class F> static void run_block(unsigned b, F f)
{
    blockIdx.x = b;
    std::barrier<> bb(64), w0(64);
    g_block_barrier = &bb;
    g_wave_barrier[0] = &w0;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 64; ++t)
        th.emplace_back([&, t] {
            threadIdx.x = t;
            f();
        });
    for (auto &t : th) t.join();
}

int main(int argc, char **argv)
{
    using namespace gnuais;
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    int64_t hd[7];
    if (fread(hd, 8, 7, f) != 7) return 3;
    const int N = (int) hd[0], n_seg = (int) hd[1], seg_words = (int) hd[2];
    const uint32_t cap = (uint32_t) hd[3];
    const int n_calls = (int) hd[4];
    const uint32_t cand_cap = (uint32_t) hd[5];
    const int blocks = (int) hd[6];
    std::vector<uint64_t> seen(N);
    if (fread(seen.data(), 8, N, f) != (size_t) N) return 4;
    std::vector<uint32_t> ctl((size_t) HDLC_CTL_WORDS * N, 0), lctl((size_t) LONG_CTL_WORDS * N, 0);
    std::vector<uint32_t> open((size_t) LONG_REC_WORDS * N, 0xdeadbeefu), clean((size_t) LONG_REC_WORDS * N, 0xdeadbeefu);
    std::vector<uint32_t> frames((size_t) cap * LONG_FRAME_WORDS, 0xdeadbeefu), cand((size_t) cand_cap * LONG_CAND_WORDS, 0xdeadbeefu);
    std::vector<int32_t> counters((size_t) 3 * N, 0);
    uint32_t count[2] = {0, 0}, cand_count[2] = {0, 0};
    int parity = 0;
    for (int c = 0; c < N; ++c) lctl[c] = 1;     // ST_SKURR: what launch_hdlc_long_reset() leaves
    blockDim.x = 64;
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
        if (cand_count[parity] != 0) return 8;  // the call before cleared this call's counter
        for (int b = 0; b < (N + 63) / 64; ++b)
            run_block((unsigned) b, [&] {
                hdlc_long_kernel<true>(segbits.data(), segcnt.data(), ctl.data(), lctl.data(), open.data(), counters.data(),
                                       frames.data(), count, cap, N, n_seg, seg_words, (int) lh[0], (long long) lh[1],
                                       clean.data(), cand.data(), cand_count, cand_cap, parity);
            });
        for (int b = 0; b < blocks; ++b)
            run_block((unsigned) b, [&] {
                hdlc_long_repair_kernel(cand.data(), cand_count + parity, cand_cap, counters.data() + (size_t) 2 * N,
                                        frames.data(), count, cap, N, blocks);
            });
        fwrite(lctl.data(), 4, lctl.size(), g);
        fwrite(cand_count + parity, 4, 1, g);
        parity ^= 1;
    }
    fwrite(counters.data(), 4, counters.size(), g);
    fwrite(count, 4, 2, g);
    fwrite(frames.data(), 4 * LONG_FRAME_WORDS, count[0] < cap ? count[0] : cap, g);
    fclose(f);
    fclose(g);
    return 0;
}
