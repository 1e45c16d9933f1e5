// long_unique_kernel_main.cpp -- TEST INFRASTRUCTURE: frame_unique.hip's own text on the CPU, over the long frames
// (tests/test_long_unique_cpu.py builds it under ASan + UBSan with tests/c/hip_cpu (serial mode) in front of the HIP and rocPRIM
// headers: the kernels have no barrier, no LDS and no cross-lane operation, so a launch is a loop over lanes), driven as
// gnuais_batch_drain_long_frames_unique / _heard drive it: the hashed attempt, the exact one when the collision word is
// set, the deliver step behind the kept attempt only, the double-buffered tail.  Drains with and without the lists
// alternate on one state.  Every buffer is allocated at exactly the size the launch interface asks for.
// argv: in out hash_bits.  in: int32 W, int32 drains, per drain int32 n, int64 rows, n records.  out: per drain int32 exact
// attempts, int32 records, int32 members (-1: no lists), int64 late so far, the records, the copies and -- with lists --
// records + 1 offsets and the members.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/gnuais_hip.h"
#include "frame_unique.hip"
using namespace gnuais;
static int bits_of(unsigned long long v) { int n = 1; while (v >> n) ++n; return n; }
// a buffer of exactly `bytes` bytes, 8-byte aligned as the interface asks (ASan sees the first byte behind it)
template <class T> static T *exact(size_t bytes) { return static_cast<T *>(bytes ? malloc(bytes) : nullptr); }
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    const int hash_bits = atoi(argv[3]);
    if (!f || !g) return 3;
    int32_t head[2];
    while (fread(head, sizeof head, 1, f) == 1) {
        uint64_t *tail = nullptr;
        int n_tail = 0;
        long long late = 0;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            const size_t N = (size_t) n;
            gnuais_long_frame *fr = exact<gnuais_long_frame>(sizeof(gnuais_long_frame) * N);
            gnuais_long_frame *out = exact<gnuais_long_frame>(sizeof(gnuais_long_frame) * N);
            int32_t *oc = exact<int32_t>(4 * N);
            if (n && fread(fr, sizeof(gnuais_long_frame), N, f) != N) return 6;
            const bool heard = (d & 1) == 0;
            int32_t *first = heard ? exact<int32_t>(4 * (N + 1)) : nullptr;
            gnuais_hearer *mem = heard ? exact<gnuais_hearer>(sizeof(gnuais_hearer) * N) : nullptr;
            char *hscratch = heard ? exact<char>(unique_heard_scratch_bytes(n)) : nullptr;
            uint32_t max_ch = 0;
            for (size_t i = 0; i < N; ++i) max_ch = fr[i].channel > max_ch ? fr[i].channel : max_ch;
            const int m = n_tail + n;
            int32_t exact_runs = 0, nm = heard ? 0 : -1;
            uint32_t np = 0;
            if (heard) first[0] = 0;
            if (m) {
                const size_t sb = unique_scratch_bytes(m, UniqueKind::Long);
                char *scratch = exact<char>(sb);
                uint64_t *next = exact<uint64_t>(sizeof(gnuais_long_frame) * (size_t) m);
                UniqueLaunch a;
                a.kind = UniqueKind::Long;
                a.frames = fr; a.have = n;
                a.tail = n_tail ? tail : nullptr; a.n_tail = n_tail; a.tail_out = next;
                a.window = head[0]; a.rows = rows; a.hash_bits = hash_bits;
                a.ch_bits = bits_of(max_ch); a.time_bits = bits_of((unsigned long long) rows);
                a.scratch = scratch; a.scratch_bytes = sb;
                a.out_frames = out; a.out_copies = oc;
                if (heard) {
                    a.heard_scratch = hscratch; a.heard_scratch_bytes = unique_heard_scratch_bytes(n);
                    a.out_first = first; a.out_members = mem;
                }
                const uint32_t *info = unique_info(a.scratch);
                for (int ex = 0; ex < 2; ++ex) {
                    if (unique_cluster_enqueue(a, ex != 0, nullptr) != hipSuccess) return 7;
                    exact_runs += ex;
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
                // the next drain sees a tail of exactly n_tail entries
                uint64_t *kept = exact<uint64_t>(sizeof(gnuais_long_frame) * (size_t) n_tail);
                if (n_tail) memcpy(kept, next, sizeof(gnuais_long_frame) * (size_t) n_tail);
                free(next);
                free(tail);
                tail = kept;
                free(scratch);
            }
            const int32_t r3[3] = {exact_runs, (int32_t) np, nm};
            const int64_t l = late;
            fwrite(r3, sizeof r3, 1, g);
            fwrite(&l, sizeof l, 1, g);
            if (np) {
                fwrite(out, sizeof(gnuais_long_frame), np, g);
                fwrite(oc, 4, np, g);
            }
            if (heard) {
                fwrite(first, 4, (size_t) np + 1, g);
                if (nm) fwrite(mem, sizeof(gnuais_hearer), (size_t) nm, g);
            }
            free(fr); free(out); free(oc); free(first); free(mem); free(hscratch);
        }
        free(tail);
    }
    fclose(f);
    fclose(g);
    return 0;
}
