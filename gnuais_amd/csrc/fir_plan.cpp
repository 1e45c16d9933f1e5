// fir_plan.cpp -- the sign-exact slicer's error bounds and the choice of the FIR kernel (fir_plan.h).
//
// The decoded bits are bit-identical to the reference's because K1s trusts the sign of its central sum y_c only where
// |y_c| > eps, and eps bounds |y_c - y_ref| for every input.  The derivation of eps is this file; its comments are the proof.
// Compile with -ffp-contract=off, like everything else that has to round as written.
#include "fir_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace gnuais {

namespace {

constexpr double u = 5.9604644775390625e-8, X = 32768.0;      // fp32 unit roundoff; |x| <= X

// An ordered fp32 sum s_1 = fl(p_1), s_j = fl(s_{j-1} + fl(p_j)) of n products carries
// product i with the factor (1+d_i) * prod_{j=max(i,2)..n} (1+e_j), |d|,|e| <= u: k_i = n
// rounding factors for i = 1, n-i+2 for i >= 2 (Higham, Accuracy and Stability, sec. 4.2).
// So |s_n - S| <= X * sum_i |t_i| * ((1+u)^k_i - 1): the late terms of the sum, and for a
// bell-shaped table the big central ones are late enough, pass through few additions.
// The reference adds in tap order (filter.h:40-49); K1s's accumulators take their NC
// products in sample order, which is tap order from one edge of the centre to the other
// (either edge: the table is symmetric).
double ordered(const float *te, int first, int n)
{
    double e = 0;
    for (int i = 1; i <= n; ++i)
        e += std::fabs((double) te[first + i - 1]) * (std::pow(1 + u, i == 1 ? n : n - i + 2) - 1);
    return e;
}

// NC = 12 is evaluated in direct form: s_q = x_a + x_b (exact: both are int16-valued), then
// y = fl(t_0 s_0), y = fl(y + fl(t_q s_q)) for q = 1..NC/2-1, edge taps first; |s_q| <= 2X: an ordered sum of NC / 2
// products of twice the size (the factor 2 is exact in every term and in the sum)
double paired(const float *te, int J0, int NC) { return 2.0 * ordered(te, J0, NC / 2); }

// The share of the bound that taps i0 .. NE (1-based, as in ordered()) carry in the reference's sum: the tap itself --
// it is outside the centre -- and its rounding factors
double ahead_from(const float *te, int NE, int i0)
{
    double a = 0;
    for (int i = i0; i <= NE; ++i)
        a += std::fabs((double) te[i - 1]) * (1.0 + (std::pow(1 + u, NE - i + 2) - 1));
    return a;
}

// eps_pk and the split bound = part_seen + part_ahead for the NC central taps from J0 on; bound_pk: the bound for the transposed sum
FirThresholds thresholds(const float *te, int NE, int J0, int NC, double bound, double bound_pk)
{
    FirThresholds t;
    t.NC = NC;
    t.eps_pk = (float) (bound_pk * 1.1);
    for (int q = 0; q < 5; ++q) {               // q < 4: the packed kernel's positions in a group; 4: any output
        const double ah = ahead_from(te, NE, J0 + NC + 1 + (q < 4 ? 6 - 2 * q : 0));
        (q < 4 ? t.eps_ahead_k[q] : t.eps_ahead) = (float) (X * ah * 1.1 + 1e-30);
        (q < 4 ? t.eps_seen_k[q] : t.eps_seen) = (float) ((bound - X * ah) * 1.1);
    }
    return t;
}

// FL2 (fir_sign_kernel): the direct form's central taps times k = 2 / P, P = the power of two at or above
// eps.  k is a power of two >= 1, so every product, pre-add and partial sum of the scaled evaluation is
// exactly k times the unscaled one (nothing overflows: |y'| <= 2 X sum|t| / eps < 1e9; an underflow the
// unscaled sum has, the scaled one has at most as badly) and |y_c| < P  <=>  |y'| < 2  <=>  exponent
// bit 7 of y' clear.  P >= eps: the band only widens.  Not taken when a central tap is subnormal or k
// would leave [1, 2^60].
float flag_scale(float eps, const float *tc, int nc)
{
    if (!(eps > 0.0f) || !(eps <= 2.0f) || !K1S_DIRECT(nc)) return 0.0f;
    int e = 0;
    const float m = std::frexp(eps, &e);            // eps = m 2^e, m in [0.5, 1)
    const float P = std::ldexp(1.0f, m == 0.5f ? e - 1 : e);
    const float k = 2.0f / P;
    if (!(k >= 1.0f) || !(k <= 1.152921504606846976e18f)) return 0.0f;
    for (int j = 0; j < nc; ++j) {
        const float t = tc[j];
        if (t != 0.0f && (!std::isnormal(t) || !std::isnormal(t * k))) return 0.0f;
    }
    return k;
}

// The 48 central taps as 24-bit integers tq = round(S t) for fir_sign_mfma.hip; false when the table does not fit (a tap
// too large for the scale or for three signed int8 digits).  bound_q: sum |tq / S - tc| (what the quantisation adds to the
// certification bound, per unit of |x|).
bool quantise_taps(const float *tc48, int *tq_out, long *sum, double *scale, double *bound_q)
{
    double sabs = 0;
    for (int q = 0; q < FIR_MFMA_NC; ++q) sabs += std::fabs((double) tc48[q]);
    if (!(sabs > 0) || !std::isfinite(sabs)) return false;
    int e = 0;
    (void) std::frexp(8388608.0 / sabs * 0.999, &e);        // the largest power of two at or below 2^23 / sum |tc| (a power of two:
    const double S = std::ldexp(1.0, e - 1);                //  tq / S is then exact in double and fp32 alike)
    long tq[FIR_MFMA_NC], sumtq = 0, sumabs = 0;
    double bq = 0;
    for (int q = 0; q < FIR_MFMA_NC; ++q) {
        tq[q] = std::lround((double) tc48[q] * S);
        sumtq += tq[q];
        sumabs += std::labs(tq[q]);
        bq += std::fabs((double) tq[q] / S - (double) tc48[q]);
    }
    if (sumabs >= 8388608 - 64) return false;
    // three signed digits, t = 65536 t2 + 256 t1 + t0 with each in [-128, 127] (fir_sign_mfma_pack lays them out), hold exactly
    // the integers from -128 * 65793 to 127 * 65793
    for (int q = 0; q < FIR_MFMA_NC; ++q)
        if (tq[q] < -128 * 65793 || tq[q] > 127 * 65793) return false;
    for (int q = 0; q < FIR_MFMA_NC; ++q) tq_out[q] = (int) tq[q];
    *sum = sumtq;
    *scale = S;
    *bound_q = bq;
    return true;
}

} // namespace

// Error budget of the NC central taps against the reference's ordered NE-term fp32 sum, for |x| <= 32768.  The smallest
// NC the kernel is built for (12, 48) whose bound stays small enough is used: 12 for the reference table
// (32 effective taps, bound 0.23), 48 for the 192 kHz table (126 taps, bound 0.87).  40 is
// evaluated on the way as the packed kernel's alternative to 48 (fir_sign_pk.hip; the 192 kHz
// table: bound 1.4, a sixth fewer multiply-adds).
SignBounds sign_bounds(const float *te, int NE)
{
    SignBounds sb;
    if (NE > FIR_MAX_NE) return sb;
    for (int j = 0; j < NE; ++j)
        if (memcmp(&te[j], &te[NE - 1 - j], 4) != 0) return sb;
    const double reference = ordered(te, 0, NE);
    for (int NC : {12, 40, 48}) {
        if (sb.ok || NE < NC || (NE - NC) % 2) continue;
        const int J0 = (NE - NC) / 2;
        double sum_out = 0;
        for (int j = 0; j < NE; ++j)
            if (j < J0 || j >= J0 + NC) sum_out += std::fabs((double) te[j]);
        // + NE subnormal products, each off by at most 2^-150 (absolute): the 1e-30
        const double transposed = ordered(te, J0, NC);
        const double central = K1S_DIRECT(NC) ? paired(te, J0, NC) : transposed;
        const double bound = X * (reference + central + sum_out) + 1e-30;
        const double bound_pk = X * (reference + transposed + sum_out) + 1e-30;    // transposed sum (fir_sign_pk.hip)
        if (!std::isfinite(bound) || !(bound < 2.0)) continue;
        // every threshold below is the bound times 1.1: headroom for this derivation's own double arithmetic and the casts to float
        if (NC == 40) {
            // the packed kernel only (running window maximum: its window behind a group is 96 rows)
            sb.ok40 = NC - 1 + J0 <= 96;
            if (sb.ok40) sb.at_40 = thresholds(te, NE, J0, NC, bound, bound_pk);
            continue;
        }
        sb.ok = true;
        sb.at_nc = thresholds(te, NE, J0, NC, bound, bound_pk);
        sb.at_nc.eps = sb.at_40.eps = (float) (bound * 1.1);
        if (NC == FIR_MFMA_NC && J0 <= 48) {
            // fir_sign_mfma.hip: the central sum in exact integer arithmetic on quantised taps -- the bound is the
            // reference's own rounding + the omitted taps + the quantisation, ALL of it per unit of the largest
            // |x| in reach of a window (its running maximum covers the rows behind and ahead), + 1 for the floor
            double bq = 0;
            if (quantise_taps(&te[J0], sb.tq, &sb.tq_sum, &sb.S, &bq)) {
                const double rel = reference + sum_out + bq;               // per unit of |x|, in units of y
                if (X * rel < 2.0) {
                    sb.mfma_ok = true;
                    sb.mfma_seen_u = (float) (rel * (sb.S / 256.0) * 1.1);
                    sb.mfma_abs_u = 3.0f;
                }
            }
        }
        if (K1S_DIRECT(NC)) sb.at_nc.fscale = flag_scale(sb.at_nc.eps, &te[J0], NC);
    }
    return sb;
}

SignChoice sign_choice(const SignBounds &sb, const FirOptions &o, int N)
{
    SignChoice c;
    c.exact = sb.ok && o.fir_variant == 3;
    c.th = sb.at_nc.NC == 48 && sb.ok40 && o.fir_pk_taps != 48 ? sb.at_40 : sb.at_nc;
    if (!o.fir_flag2) c.th.fscale = 0.0f;
    c.eps = c.th.fscale > 0.0f ? 2.0f / c.th.fscale : c.th.eps;
    c.matrix_pipe = o.fir_mfma && sb.mfma_ok && N % 64 == 0 && o.fir_variant == 3;
    return c;
}

FirPlan plan_fir(const SignBounds &sb, const FirOptions &o, const FirShape &s, int len, bool dump)
{
    const SignChoice c = sign_choice(sb, o, s.N);
    auto whole = [](int v, int q) { return std::min((v + q - 1) / q * q, FIR_MAX_T / q * q); };     // whole quanta, at most FIR_MAX_T
    FirPlan p;
    if (!c.exact || dump) {         // the exact kernels take no threshold; their launch carries at_nc's eps_pk and split
        p.kernel = s.NE != 32 ? FirKernel::GENERIC : FirKernel::SCALAR32;
        p.th.NC = sb.at_nc.NC, p.th.T = o.fir_T, p.th.eps = sb.at_nc.eps, p.th.eps_pk = sb.at_nc.eps_pk;
        p.th.eps_seen = sb.at_nc.eps_seen, p.th.eps_ahead = sb.at_nc.eps_ahead;
        return p;
    }
    p.th = c.th;
    const int NC = p.th.NC;
    // 12 central taps, or a window behind a group of more than 96 rows: fir_slice.hip, whole turns of its unrolled body
    p.kernel = FirKernel::SIGN;
    p.th.T = whole(o.fir_T, K1S_DIRECT(NC) ? FIR_Q_SIGN12 : FIR_Q_SIGN48);
    if (K1S_DIRECT(NC) || NC - 1 + (s.NE - NC) / 2 > 96) return p;
    // 40 / 48 central taps (the 192 kHz table): the transposed sum on register pairs (fir_sign_pk.hip)
    const int qp = NC == 40 ? FIR_Q_PK40 : FIR_Q_PK48;
    // 48 taps: a segment's warm-up is 47 pair steps' worth of samples; longer segments (there are plenty of
    // waves: 16384 x 192000 is 16000 segments of 3072) cut its share (round 4: 3072 against 1536, 4.29 against
    // 4.39 ms per C5 call in steady state, profiles/r04_c5_ring_and_segments.txt)
    // 40 taps: 1920 (FIR alone 3.34-3.40 ms against 3.43-3.49 at 3200 and 3.85 at 6400: the lists of open outputs a
    // segment settles at its end grow with it; profiles/r05_c5_forty_central_taps.txt)
    p.th.T = whole(o.fir_T <= 768 ? (NC == 40 ? 1920 : 3072) : o.fir_T, qp);
    // The matrix-pipe kernel takes everything but the call's head -- the outputs whose windows reach into the history
    // rows --, which stays the packed kernel's: the fewest whole packed loop turns (and whole 16-byte sign stores) that
    // cover d and dc + 64 rows (640 outputs for the 192 kHz table: one wave per 64 channels walks it alone, 0.1 ms for
    // 256 waves on 1024 SIMDs; round 5's whole first segment of 1920 took 0.3).  (Beside the matrix-pipe launch on a side
    // stream, between two events: 2.44 instead of 2.51 ms per C5 call, but one pipelined run in six came out with a frame
    // more or less -- not kept; profiles/r06_c5_matrix_pipe_k32.txt.)
    const int dc48 = s.d - (s.NE - FIR_MFMA_NC) / 2, qh = std::lcm(qp, FIR_Q_MFMA);
    const int head = (std::max(dc48 + 64, s.d) + qh - 1) / qh * qh;
    // the last condition is the kernel's 31-bit buffer offsets: per call, so not part of SignChoice::matrix_pipe
    const bool mfma = c.matrix_pipe && p.th.T % FIR_Q_MFMA == 0 && len > head && len >= s.NT && head <= FIR_MAX_T &&
                      (unsigned long long) (p.th.T + s.NE + 512) * (unsigned long long) s.N * 2ull < 0x7fffffffull;
    p.kernel = mfma ? FirKernel::SIGN_PACKED_MFMA : FirKernel::SIGN_PACKED;
    if (mfma) p.head = head, p.mfma_seen_u = sb.mfma_seen_u, p.mfma_abs_u = sb.mfma_abs_u;
    return p;
}

} // namespace gnuais
