// heard_main.cpp -- TEST INFRASTRUCTURE: the host object's gnuais_uniq_push_heard by itself (tests/test_heard_cpu.py builds
// it with frame_unique.cpp under ASan + UBSan; no HIP, nothing loaded into Python).  push and push_heard alternate on one
// object, drain by drain; every buffer is allocated at exactly the size the interface asks for.
// argv: in out.  in: int32 W, int32 drains, int32 with_signal, per drain int32 n, int64 rows, n records, n times, n signal
// records.  out: per drain int32 rc, int32 records, int32 members (-1: a plain push), int64 late so far, the records,
// times, copies and -- behind a push_heard -- records + 1 offsets and the members.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnuais_hip.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    static_assert(sizeof(gnuais_hearer) == 24, "gnuais_hearer is 24 bytes");
    int32_t head[3];
    while (fread(head, sizeof head, 1, f) == 1) {
        gnuais_uniq *u = nullptr;
        if (gnuais_uniq_create(&u, head[0]) != GNUAIS_OK) return 4;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            const size_t N = (size_t) n;
            std::vector<gnuais_frame> fr(N), out(N);
            std::vector<int64_t> tm(N), ot(N);
            std::vector<gnuais_frame_signal> sg(N);
            std::vector<int32_t> oc(N), first(N + 1);
            std::vector<gnuais_hearer> mem(N);
            if (n && (fread(fr.data(), sizeof(gnuais_frame), N, f) != N || fread(tm.data(), 8, N, f) != N ||
                      fread(sg.data(), sizeof(gnuais_frame_signal), N, f) != N))
                return 6;
            int got = -1, nm = -1;
            const bool heard = (d & 1) == 0;
            const int32_t rc = heard ? gnuais_uniq_push_heard(u, fr.data(), tm.data(), head[2] ? sg.data() : nullptr, n, rows,
                                                              out.data(), ot.data(), oc.data(), n, &got, first.data(),
                                                              mem.data(), &nm)
                                     : gnuais_uniq_push(u, fr.data(), tm.data(), n, rows, out.data(), ot.data(), oc.data(), n, &got);
            const int32_t r3[3] = {rc, got, nm};
            const int64_t late = gnuais_uniq_late(u);
            fwrite(r3, sizeof r3, 1, g);
            fwrite(&late, sizeof late, 1, g);
            if (got > 0) {
                fwrite(out.data(), sizeof(gnuais_frame), (size_t) got, g);
                fwrite(ot.data(), 8, (size_t) got, g);
                fwrite(oc.data(), 4, (size_t) got, g);
            }
            if (heard) {
                fwrite(first.data(), 4, (size_t) got + 1, g);
                if (nm > 0) fwrite(mem.data(), sizeof(gnuais_hearer), (size_t) nm, g);
            }
        }
        gnuais_uniq_destroy(u);
    }
    int got = 0, nm = 0;
    int32_t one = 7;
    if (gnuais_uniq_push_heard(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, &got, &one, nullptr, &nm) != GNUAIS_E_ARG)
        return 9;
    fclose(f);
    fclose(g);
    return 0;
}
