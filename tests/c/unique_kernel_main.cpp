// unique_kernel_main.cpp -- TEST INFRASTRUCTURE: frame_unique.hip's own text on the CPU (tests/test_unique_cpu.py builds it
// under ASan + UBSan with tests/c/hip_cpu (serial mode) in front of the HIP and rocPRIM headers), driven as
// gnuais_batch_drain_frames_unique drives it: the hashed attempt, the exact one when the collision word is set, the
// double-buffered tail.  Every buffer is allocated at exactly the size the launch interface asks for.
// argv: in out hash_bits.  in: int32 W, int32 drains, per drain int32 n, int64 rows, n records, n times.
// out: per drain int32 exact attempts, int32 records, int64 late so far, the records, times and copies.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/gnuais_hip.h"
#include "frame_unique.hip"
using namespace gnuais;
static int bits_of(unsigned long long v) { int n = 1; while (v >> n) ++n; return n; }
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    const int hash_bits = atoi(argv[3]);
    if (!f || !g) return 3;
    int32_t head[2];
    while (fread(head, sizeof head, 1, f) == 1) {
        std::vector<uint32_t> tail;
        int n_tail = 0;
        long long late = 0;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            std::vector<gnuais_frame> fr((size_t) n), out((size_t) n);
            std::vector<int64_t> tm((size_t) n), ot((size_t) n);
            std::vector<int32_t> oc((size_t) n);
            if (n && (fread(fr.data(), sizeof(gnuais_frame), (size_t) n, f) != (size_t) n || fread(tm.data(), 8, (size_t) n, f) != (size_t) n)) return 6;
            uint32_t max_ch = 0;
            for (const gnuais_frame &x : fr) max_ch = x.channel > max_ch ? x.channel : max_ch;
            const int m = n_tail + n;
            int32_t exact_runs = 0;
            uint32_t np = 0;
            if (m) {
                std::vector<char> scratch(unique_scratch_bytes(m));
                std::vector<uint32_t> next((size_t) 16 * m);
                UniqueLaunch a;
                a.frames = fr.data(); a.times = tm.data(); a.have = n;
                a.tail = n_tail ? tail.data() : nullptr; a.n_tail = n_tail; a.tail_out = next.data();
                a.window = head[0]; a.rows = rows; a.hash_bits = hash_bits;
                a.ch_bits = bits_of(max_ch); a.time_bits = bits_of((unsigned long long) rows);
                a.scratch = scratch.data(); a.scratch_bytes = scratch.size();
                a.out_frames = out.data(); a.out_times = ot.data(); a.out_copies = oc.data();
                const uint32_t *info = unique_info(a.scratch);
                for (int exact = 0; exact < 2; ++exact) {
                    if (unique_cluster_enqueue(a, exact != 0, nullptr) != hipSuccess) return 7;
                    exact_runs += exact;
                    if (!info[UNIQUE_INFO_COLLISION]) break;
                }
                np = info[UNIQUE_INFO_PRIMARIES];
                if (np > (uint32_t) n || info[UNIQUE_INFO_TAIL] > (uint32_t) m) return 8;
                if (unique_deliver_enqueue(a, (int) np, nullptr) != hipSuccess) return 9;
                unsigned long long add = 0;
                memcpy(&add, info + UNIQUE_INFO_LATE, sizeof add);
                late += (long long) add;
                n_tail = (int) info[UNIQUE_INFO_TAIL];
                next.resize((size_t) 16 * n_tail);
                tail.swap(next);
            }
            const int32_t r2[2] = {exact_runs, (int32_t) np};
            const int64_t l = late;
            fwrite(r2, sizeof r2, 1, g);
            fwrite(&l, sizeof l, 1, g);
            if (np) {
                fwrite(out.data(), sizeof(gnuais_frame), np, g);
                fwrite(ot.data(), 8, np, g);
                fwrite(oc.data(), 4, np, g);
            }
        }
    }
    fclose(f);
    fclose(g);
    return 0;
}
