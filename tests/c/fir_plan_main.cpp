// fir_plan_main.cpp -- TEST INFRASTRUCTURE: drives gnuais_amd/csrc/fir_plan.cpp on the CPU (tests/test_fir_plan_cpu.py).
//
//   fir_plan.bin FILE      FILE: lines of
//       table NAME NT d NE <NE taps as hex words>                               -> bounds name=NAME k=v ...
//       plan N len fir_variant fir_T fir_pk_taps fir_flag2 fir_mfma dump        -> plan k=v ... (for the last table)
// Floats are printed as C hex floats.  The taps live in a heap block of exactly NE floats -- none at all for a table
// beyond FIR_MAX_NE -- so that a read past the input is the sanitizers' to find.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gnuais_amd/csrc/fir_plan.h"

using namespace gnuais;

static void pf(const char *k, float v) { printf(" %s=%a", k, (double) v); }
static void pf4(const char *k, const float *v) { printf(" %s=%a,%a,%a,%a", k, (double) v[0], (double) v[1], (double) v[2], (double) v[3]); }

int main(int argc, char **argv)
{
    FILE *in = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!in) return 2;
    static const char *kernels[] = {"generic", "scalar32", "sign", "packed", "packed+mfma"};
    char word[64], name[64];
    SignBounds sb;
    FirShape shape = {0, 0, 0, 0};
    bool have = false;
    while (fscanf(in, "%63s", word) == 1) {
        if (!strcmp(word, "table")) {
            if (fscanf(in, "%63s %d %d %d", name, &shape.NT, &shape.d, &shape.NE) != 4 || shape.NE < 1) return 3;
            std::vector<float> te;
            for (int j = 0; j < shape.NE; ++j) {
                uint32_t w;
                float t;
                if (fscanf(in, "%x", &w) != 1) return 3;
                memcpy(&t, &w, 4);
                if (shape.NE <= FIR_MAX_NE) te.push_back(t);
            }
            te.shrink_to_fit();
            sb = sign_bounds(te.empty() ? nullptr : te.data(), shape.NE);
            have = true;
            const FirThresholds &t = sb.at_nc, &t40 = sb.at_40;
            printf("bounds name=%s ok=%d NC=%d", name, (int) sb.ok, t.NC);
            pf("eps", t.eps); pf("eps_pk", t.eps_pk); pf("seen", t.eps_seen); pf("ahead", t.eps_ahead);
            pf("fscale", t.fscale); pf4("seen_k", t.eps_seen_k); pf4("ahead_k", t.eps_ahead_k);
            printf(" ok40=%d", (int) sb.ok40);
            pf("eps_pk40", t40.eps_pk); pf("seen40", t40.eps_seen); pf("ahead40", t40.eps_ahead);
            pf4("seen_k40", t40.eps_seen_k); pf4("ahead_k40", t40.eps_ahead_k);
            printf(" mfma_ok=%d", (int) sb.mfma_ok);
            pf("mfma_seen_u", sb.mfma_seen_u); pf("mfma_abs_u", sb.mfma_abs_u);
            printf(" S=%a k0=%d tq=", sb.S, (int) (128 * sb.tq_sum));
            for (int q = 0; q < FIR_MFMA_NC; ++q) printf("%s%d", q ? "," : "", sb.tq[q]);
            printf("\n");
        } else if (!strcmp(word, "plan")) {
            FirOptions o;
            int len, dump;
            if (!have || fscanf(in, "%d %d %d %d %d %d %d %d", &shape.N, &len, &o.fir_variant, &o.fir_T, &o.fir_pk_taps, &o.fir_flag2,
                                &o.fir_mfma, &dump) != 8)
                return 4;
            const FirPlan p = plan_fir(sb, o, shape, len, dump != 0);
            const FirThresholds &t = p.th;
            printf("plan kernel=%s NC=%d T=%d head=%d", kernels[(int) p.kernel], t.NC, t.T, p.head);
            pf("eps", t.eps); pf("eps_pk", t.eps_pk); pf("eps_seen", t.eps_seen); pf("eps_ahead", t.eps_ahead); pf("fscale", t.fscale);
            pf4("seen_k", t.eps_seen_k); pf4("ahead_k", t.eps_ahead_k); pf("mfma_seen_u", p.mfma_seen_u); pf("mfma_abs_u", p.mfma_abs_u);
            // what gnuais_batch_info() answers for the names of these keys
            const SignChoice c = sign_choice(sb, o, shape.N);
            printf(" sign_exact=%a sign_central_taps=%a sign_eps=%a sign_flag_scale=%a sign_eps_seen=%a sign_eps_ahead=%a sign_matrix_pipe=%a\n",
                   (double) c.exact, (double) c.th.NC, (double) c.eps, (double) c.th.fscale, (double) c.th.eps_seen, (double) c.th.eps_ahead,
                   (double) c.matrix_pipe);
        } else {
            return 5;
        }
    }
    fclose(in);
    return 0;
}
