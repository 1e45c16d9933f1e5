// occupancy_kernel_main.cpp -- TEST INFRASTRUCTURE: the three kernels of occupancy.hip, their own text, on the CPU
// (tests/test_occupancy_cpu.py builds it under ASan + UBSan with tests/c/hip_cpu in front of the HIP headers).  Every
// buffer has exactly the size its launch is given.  The finaliser runs through launch_occ_epoch().  The code and cover
// kernels are launched on grids smaller than the library's, which makes their grid-stride loops turn; for the first epoch
// launch_occ_code() and launch_occ_cover() run as well, on copies of the same input, and must leave the same bytes.
// argv: in out.  in: int64 N, E, margin, CB, n_epochs, n_frames, pllinc, n_taps, W, v0; P int64 [n_epochs * E][N]; frames
// int64 [n_frames][3] = channel, nbits, t.  The epochs are made final one by one, each by the shortest call that does so.
// out, per epoch: the records [N], the tap words [E][N], the carried busy bytes [N].
#include <hip/hip_runtime.h>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "occupancy.hip"

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
    std::vector<int64_t> times((size_t) n_frames);
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
        std::vector<uint16_t> codes_lib(codes);
        std::vector<uint8_t> cover_lib(cover);
        const int n_groups = (N + 255) / 256, stride = 3;
        hipLaunchKernelGGL(occ_code_kernel, dim3((unsigned) (n_groups * stride)), dim3(OCC_THREADS), 0, nullptr, sums.data(), RB,
                           codes.data(), CB, N, first, E, n_groups, stride);
        OccCoverLaunch a;
        a.frames = frames.data(); a.frame_count = count.data(); a.frame_cap = (uint32_t) n_frames; a.times = times.data();
        a.cover = cover.data(); a.CB = CB; a.N = N; a.len = (int) (end - n0); a.n0 = n0; a.pllinc = pllinc; a.n_taps = n_taps;
        a.afc_window = W; a.v0 = v0; a.b0 = b0;
        hipLaunchKernelGGL(occ_cover_kernel, dim3(2), dim3(OCC_THREADS), 0, nullptr, (const uint32_t *) a.frames, a.frame_count,
                           a.frame_cap, (const long long *) a.times, a.cover, a.CB, a.N, (long long) a.n0, a.len, a.pllinc,
                           a.n_taps, a.afc_window, (long long) a.v0, (long long) a.b0);
        if (k == 0) {
            a.cover = cover_lib.data();
            if (launch_occ_code(sums.data(), RB, codes_lib.data(), CB, N, first, E, nullptr) != hipSuccess ||
                launch_occ_cover(a, nullptr) != hipSuccess)
                return 6;
            if (codes_lib != codes || cover_lib != cover) return 7;
        }
        OccEpochLaunch e;
        e.codes = codes.data(); e.cover = cover.data(); e.carry = carry.data(); e.out = out.data();
        e.CB = CB; e.N = N; e.E = E; e.margin = margin; e.first = first; e.first_epoch = k == 0;
        if (launch_occ_epoch(e, nullptr) != hipSuccess) return 8;
        fwrite(out.data(), 8, (size_t) N, g);
        for (int i = 0; i < E; ++i) fwrite(codes.data() + (size_t) ((first + i) % CB) * N, 2, (size_t) N, g);
        fwrite(carry.data(), 1, (size_t) N, g);
        n0 = end;
    }
    fclose(g);
    printf("epochs: %d\n", n_epochs);
    return 0;
}
