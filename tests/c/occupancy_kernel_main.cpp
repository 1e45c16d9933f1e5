// occupancy_kernel_main.cpp -- TEST INFRASTRUCTURE: the three kernels of occupancy.hip, their own text, on the CPU
// (tests/test_occupancy_cpu.py builds it under ASan + UBSan with tests/c/hip_grid_shim in front of the HIP headers): a
// std::thread per lane, one block at a time.  OCC_KERNEL_TEXT is a copy of occupancy.hip whose dynamic shared array is an
// ordinary declaration.  Every buffer has exactly the size its launch is given.
// argv: in out.  in: int64 N, E, margin, CB, n_epochs, n_frames, pllinc, n_taps, W, v0; P int64 [n_epochs * E][N]; frames
// int64 [n_frames][3] = channel, nbits, t.  The epochs are made final one by one, each by the shortest call that does so.
// out, per epoch: the records [N], the tap words [E][N], the carried busy bytes [N].
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
constexpr int LDS_WORDS = 288 * 32 + 256 + 64 + 3 * 256;
namespace gnuais { namespace { uint32_t occ_lds[LDS_WORDS]; } }
#include OCC_KERNEL_TEXT
static_assert(LDS_WORDS == gnuais::OCC_LDS_WORDS, "the finaliser's launch size");

// `blocks` blocks of 256 threads, one block at a time
static void run_grid(unsigned blocks, const std::function<void()> &kernel)
{
    gridDim.x = blocks;
    for (unsigned b = 0; b < blocks; ++b) {
        blockIdx.x = b;
        std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
        g_block_barrier = &bb;
        g_wave_barrier[0] = &w0; g_wave_barrier[1] = &w1; g_wave_barrier[2] = &w2; g_wave_barrier[3] = &w3;
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
    int64_t hd[10];
    if (fread(hd, 8, 10, f) != 10) return 3;
    const int N = (int) hd[0], E = (int) hd[1], margin = (int) hd[2], CB = (int) hd[3], n_epochs = (int) hd[4];
    const int n_frames = (int) hd[5], n_taps = (int) hd[7], W = (int) hd[8];
    const uint32_t pllinc = (uint32_t) hd[6];
    const long long v0 = hd[9], b0 = (v0 + 63) / 64;
    std::vector<int64_t> P((size_t) n_epochs * E * N), fr((size_t) n_frames * 3);
    if (fread(P.data(), 8, P.size(), f) != P.size() || fread(fr.data(), 8, fr.size(), f) != fr.size()) return 4;
    fclose(f);

    const int RB = E;
    std::vector<int64_t> sums((size_t) RB * N * 3, -12345);
    std::vector<uint16_t> codes((size_t) CB * N, 0xffff);
    std::vector<uint8_t> cover((size_t) CB * N, 0), carry((size_t) N, 0xaa);
    std::vector<uint2> out((size_t) N);
    std::vector<uint32_t> frames((size_t) n_frames * 16, 0xdeadbeef), count(4, 0);
    std::vector<long long> times((size_t) n_frames);
    for (int i = 0; i < n_frames; ++i) {
        frames[(size_t) i * 16] = (uint32_t) fr[(size_t) i * 3];
        frames[(size_t) i * 16 + 15] = (uint32_t) fr[(size_t) i * 3 + 1] << 16 | 0xbeefu;
        times[(size_t) i] = fr[(size_t) i * 3 + 2];
    }
    count[0] = (uint32_t) n_frames;

    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    const long long lag = occ_lag_rows(pllinc, n_taps, W);
    long long n0 = v0;
    for (int k = 0; k < n_epochs; ++k) {
        const long long first = b0 + (long long) k * E, end = 64 * (first + E) + lag;
        for (int i = 0; i < E; ++i)
            for (int c = 0; c < N; ++c)
                sums[((size_t) ((first + i) % RB) * N + c) * 3] = P[((size_t) k * E + i) * N + c];
        const int n_groups = (N + 255) / 256, stride = 3;
        run_grid((unsigned) (n_groups * stride),
                 [&] { occ_code_kernel(sums.data(), RB, codes.data(), CB, N, first, E, n_groups, stride); });
        run_grid(2, [&] {
            occ_cover_kernel(frames.data(), count.data(), (uint32_t) n_frames, times.data(), cover.data(), CB, N, n0,
                             (int) (end - n0), pllinc, n_taps, W, v0, b0);
        });
        run_grid((unsigned) ((N + 63) / 64),
                 [&] { occ_epoch_kernel(codes.data(), cover.data(), carry.data(), out.data(), CB, N, E, margin, first, k == 0); });
        fwrite(out.data(), 8, (size_t) N, g);
        for (int i = 0; i < E; ++i) fwrite(codes.data() + (size_t) ((first + i) % CB) * N, 2, (size_t) N, g);
        fwrite(carry.data(), 1, (size_t) N, g);
        n0 = end;
    }
    fclose(g);
    printf("epochs: %d\n", n_epochs);
    return 0;
}
