// message_kernel_main.cpp -- TEST INFRASTRUCTURE: nmea_device.hip's own text on the CPU (tests/test_message_kernel_cpu.py
// builds it under ASan + UBSan with tests/c/hip_cpu in front of the HIP and rocPRIM headers).
//   argv: frames in out   the launch interface as the drain drives it, every buffer of exactly the size it asks for.
//         in:  int32 groups; per group int32 n, u8 seq_in[8], char chanid[8], n records.
//         out: per group u32 totals[4], the sentences, u8 seq_out[8], u32 info2[2], the lines, u32 vessels, the table.
//   argv: sweep stride    LineOut::fixed and ::dec called directly, against snprintf; prints the values compared.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "nmea_device.hip"
// frame_time.hip's, behind frames_sort_timed(..., times != nullptr), which this program never calls
hipError_t gnuais::launch_frame_times_gather(const int64_t *, const uint32_t *, int, int64_t *, hipStream_t) { abort(); }
using namespace gnuais;

static constexpr int N_CH = 8;

template <class T> static T *exact(size_t count)      // malloc: ASan sees one element past the end
{
    return static_cast<T *>(malloc(sizeof(T) * count));
}

static int run_frames(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb"), *g = fopen(out, "wb");
    int32_t groups;
    if (!f || !g || fread(&groups, 4, 1, f) != 1) return 2;
    for (int k = 0; k < groups; ++k) {
        int32_t n;
        uint8_t seq_in[N_CH];
        char chanid[N_CH];
        if (fread(&n, 4, 1, f) != 1 || fread(seq_in, 1, N_CH, f) != N_CH || fread(chanid, 1, N_CH, f) != N_CH || n <= 0) return 3;
        gnuais_frame *frames = exact<gnuais_frame>(n);
        if (fread(frames, sizeof *frames, n, f) != (size_t) n) return 4;
        const size_t scratch_bytes = nmea_scratch_bytes(n, 0), nmea_cap = (size_t) 164 * n, text_cap = (size_t) 512 * n;
        void *scratch = malloc(scratch_bytes);
        char *nmea = exact<char>(nmea_cap), *lines = exact<char>((size_t) n * messages_line_bytes()), *text = exact<char>(text_cap);
        uint32_t *len = exact<uint32_t>(n), *off = exact<uint32_t>(n), *info2 = exact<uint32_t>(2), *count = exact<uint32_t>(1);
        uint8_t *seq_out = exact<uint8_t>(N_CH);
        memcpy(seq_out, seq_in, N_CH);
        uint32_t totals[4] = {9, 9, 9, 9};
        if (nmea_format_enqueue(frames, n, n, N_CH, seq_in, seq_out, nmea, nmea_cap, scratch, scratch_bytes, totals, nullptr, 0, 0,
                                nullptr, nullptr) != hipSuccess) return 5;
        if (messages_format_enqueue(frames, n, N_CH, seq_in, chanid, scratch, scratch_bytes, lines, len, off, text, text_cap, info2,
                                    nullptr) != hipSuccess) return 6;
        if (totals[3] || (size_t) totals[0] + totals[1] > nmea_cap || info2[0] > text_cap) return 8;
        fwrite(totals, 4, 4, g);
        fwrite(nmea, 1, (size_t) totals[0] + totals[1], g);
        fwrite(seq_out, 1, N_CH, g);
        fwrite(info2, 4, 2, g);
        fwrite(text, 1, info2[0], g);
        // the vessel table of the same frames, on the same scratch
        gnuais_vessel *table = exact<gnuais_vessel>(n);
        if (vessels_fold_enqueue(frames, n, scratch, scratch_bytes, table, n, count, nullptr) != hipSuccess) return 9;
        if (*count > (uint32_t) n) return 10;
        fwrite(count, 4, 1, g);
        fwrite(table, sizeof *table, *count, g);
        free(frames); free(scratch); free(nmea); free(lines); free(text); free(len); free(off); free(info2); free(count);
        free(seq_out); free(table);
    }
    fclose(f);
    fclose(g);
    return 0;
}

// ---- LineOut by itself -------------------------------------------------------------------------------------------
static long long g_compared, g_wrong;

static void check(const LineOut &o, const char *got, const char *want, const char *what, double d)
{
    ++g_compared;
    const size_t n = strlen(want);
    if ((size_t) o.n == n && !memcmp(got, want, n)) return;
    if (++g_wrong <= 20) fprintf(stderr, "%s %.17g: got %.*s want %s\n", what, d, o.n, got, want);
}

static void fixed_is_printf(double d, int prec, const char *what)
{
    char got[MSG_LINE_MAX], want[64];
    LineOut o{got, 0};
    o.fixed(d, prec);
    snprintf(want, sizeof want, "%.*f", prec, d);
    check(o, got, want, what, d);
}

static void dec_is_printf(long long v, int width)
{
    char got[MSG_LINE_MAX], want[64];
    LineOut o{got, 0};
    o.dec(v, width);
    snprintf(want, sizeof want, "%0*lld", width, v);
    check(o, got, want, "dec", (double) v);
}

static void coordinates(int v)
{
    fixed_is_printf((double) (float) v / 600000.0, 6, "v / 600000.0");                              // types 1-3, 18
    fixed_is_printf((double) (float) ((double) (float) v / 10000.0 / 60.0), 6, "type 4");           // protodec_4
    fixed_is_printf((double) (float) v / 60000.0, 6, "v / 60000.0");                                // the weather report
}

static int count_of(const LineOut &o, const char *buf, const char *word)
{
    const std::string s(buf, (size_t) o.n);
    int c = 0;
    for (size_t p = s.find(word); p != std::string::npos; p = s.find(word, p + 1)) ++c;
    return c;
}

static int run_sweep(int stride)
{
    if (stride < 1 || stride % 2 == 0) return 2;
    const int dense = 1 << 21, top = 1 << 27;
    for (int v = -dense; v <= dense; ++v) coordinates(v);
    for (int v = dense + 1; v <= top; v += stride) { coordinates(v); coordinates(-v); }
    coordinates(top); coordinates(-top);
    // every %.1f expression of the file over its field's whole range
    for (int v = 0; v < 2048; ++v) fixed_is_printf((double) (float) v / 10.0 - 60.0, 1, "air_temp");
    for (int v = 0; v < 1024; ++v) fixed_is_printf((double) (float) v / 10.0 - 20.0, 1, "dew_point");
    for (int v = 0; v < 1024; ++v) fixed_is_printf((double) (float) v / 10.0 - 10.0, 1, "water_level / water_temp");
    for (int v = 0; v < 256; ++v) fixed_is_printf((double) (float) v / 10.0, 1, "visib / wave_height");
    for (int v = 0; v < 256; ++v) fixed_is_printf((double) (float) (unsigned char) v / 10.0, 1, "draught");
    for (int c = 0; c < 65536; ++c) {
        fixed_is_printf((double) (float) (unsigned short) c / 10.0, 0, "course");
        fixed_is_printf((double) (float) (unsigned short) c / 10.0, 1, "speed");
    }
    for (int width : {0, 2, 9}) {
        long long p = 1;
        for (int k = 0; k <= 18; ++k) {
            for (long long v : {p - 1, p, -(p - 1), -p}) dec_is_printf(v, width);
            if (k < 18) p *= 10;
        }
        for (long long v : {0ll, 1ll, -1ll, 2147483647ll, -2147483648ll, 4294967295ll, 4294967296ll, -4294967296ll})
            dec_is_printf(v, width);
    }
    // the two loops whose turns depend on the padded length (protodec.c:558 "pos + 32 <= bufferlen", :690 "pos + 30 <
    // bufferlen"), at every length -- a frame's own padded length is a multiple of 6 and never meets 40 + 30 i
    FrameView fv;
    for (int q = 0; q < 16; ++q) fv.w[q] = 0x5a5a5a5au;
    fv.w[15] = 424u << 16;
    const BitsView bits(fv);
    for (int padded = 0; padded <= 200; ++padded) {
        char buf[MSG_LINE_MAX];
        int acks = 0, slots = 0;
        for (int i = 0; i < 4; ++i) { acks += 40 + 32 * i + 32 <= padded; slots += 40 + 30 * i + 30 < padded; }
        LineOut a{buf, 0};
        describe_dev(bits, 7, padded, a);
        g_compared++;
        if (count_of(a, buf, " ack ") != acks && ++g_wrong <= 20) fprintf(stderr, "type 7 at %d: %.*s\n", padded, a.n, buf);
        LineOut b{buf, 0};
        describe_dev(bits, 20, padded, b);
        g_compared++;
        if (count_of(b, buf, " reserve ") != slots && ++g_wrong <= 20) fprintf(stderr, "type 20 at %d: %.*s\n", padded, b.n, buf);
    }
    printf("%lld compared, %lld wrong\n", g_compared, g_wrong);
    return g_wrong ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "frames")) return run_frames(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "sweep")) return run_sweep(atoi(argv[2]));
    return 2;
}
