// heard_kernel_main.cpp -- TEST INFRASTRUCTURE: frame_unique.hip's own text on the CPU with the member lists wanted
// (tests/test_heard_cpu.py builds it under ASan + UBSan with tests/c/hip_cpu (serial mode) in front of the HIP and rocPRIM
// headers), driven as gnuais_batch_drain_frames_heard drives it: the hashed attempt, the exact one when the collision
// word is set, the lists behind the kept attempt only, the double-buffered tail.  Drains with and without the lists
// alternate on one state.  Every buffer is allocated at exactly the size the launch interface asks for; the members
// at the 16-byte alignment it asks for.
// argv: in out hash_bits.  in: int32 W, int32 drains, int32 with_signal, per drain int32 n, int64 rows, n records, n
// times, n signal records.  out: per drain int32 exact attempts, int32 records, int32 members (-1: no lists), int64 late
// so far, the records, times, copies and -- with lists -- records + 1 offsets and the members.
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
    int32_t head[3];
    while (fread(head, sizeof head, 1, f) == 1) {
        std::vector<uint32_t> tail;
        int n_tail = 0;
        long long late = 0;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            const size_t N = (size_t) n;
            std::vector<gnuais_frame> fr(N), out(N);
            std::vector<int64_t> tm(N), ot(N);
            std::vector<gnuais_frame_signal> sg(N);
            std::vector<int32_t> oc(N);
            if (n && (fread(fr.data(), sizeof(gnuais_frame), N, f) != N || fread(tm.data(), 8, N, f) != N ||
                      fread(sg.data(), sizeof(gnuais_frame_signal), N, f) != N))
                return 6;
            const bool heard = (d & 1) == 0;
            std::vector<int32_t> first(heard ? N + 1 : 0);
            std::vector<char> hscratch(heard ? unique_heard_scratch_bytes(n) : 0);
            void *mem = nullptr;
            if (heard && n && posix_memalign(&mem, 16, sizeof(gnuais_hearer) * N)) return 10;
            uint32_t max_ch = 0;
            for (const gnuais_frame &x : fr) max_ch = x.channel > max_ch ? x.channel : max_ch;
            const int m = n_tail + n;
            int32_t exact_runs = 0, nm = heard ? 0 : -1;
            uint32_t np = 0;
            if (heard) first[0] = 0;
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
                if (heard) {
                    a.signal = head[2] ? sg.data() : nullptr;
                    a.heard_scratch = hscratch.data(); a.heard_scratch_bytes = hscratch.size();
                    a.out_first = first.data(); a.out_members = static_cast<gnuais_hearer *>(mem);
                }
                const uint32_t *info = unique_info(a.scratch);
                for (int exact = 0; exact < 2; ++exact) {
                    if (unique_cluster_enqueue(a, exact != 0, nullptr) != hipSuccess) return 7;
                    exact_runs += exact;
                    if (!info[UNIQUE_INFO_COLLISION]) break;
                }
                np = info[UNIQUE_INFO_PRIMARIES];
                if (np > (uint32_t) n || info[UNIQUE_INFO_TAIL] > (uint32_t) m) return 8;
                if (unique_deliver_enqueue(a, (int) np, nullptr) != hipSuccess) return 9;
                if (heard && np) nm = first[np];
                if (nm > n) return 11;
                unsigned long long add = 0;
                memcpy(&add, info + UNIQUE_INFO_LATE, sizeof add);
                late += (long long) add;
                n_tail = (int) info[UNIQUE_INFO_TAIL];
                next.resize((size_t) 16 * n_tail);
                tail.swap(next);
            }
            const int32_t r3[3] = {exact_runs, (int32_t) np, nm};
            const int64_t l = late;
            fwrite(r3, sizeof r3, 1, g);
            fwrite(&l, sizeof l, 1, g);
            if (np) {
                fwrite(out.data(), sizeof(gnuais_frame), np, g);
                fwrite(ot.data(), 8, np, g);
                fwrite(oc.data(), 4, np, g);
            }
            if (heard) {
                fwrite(first.data(), 4, (size_t) np + 1, g);
                if (nm) fwrite(mem, sizeof(gnuais_hearer), (size_t) nm, g);
            }
            free(mem);
        }
    }
    fclose(f);
    fclose(g);
    return 0;
}
