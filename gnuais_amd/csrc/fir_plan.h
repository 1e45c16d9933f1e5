// fir_plan.h -- what the host decides about K1 before it launches anything: the sign-exact slicer's error bounds for a
// tap table (sign_bounds) and, per call, which FIR kernel runs with which thresholds (plan_fir).  Plain C++: no HIP, no
// device state, pure functions -- the CPU tests drive them directly (tests/test_fir_plan_cpu.py).
#pragma once

namespace gnuais {

// K1s evaluates the NC = 12 central taps in direct form with symmetric pre-adds (fir_slice.hip); the
// bound for y_c follows the same order of operations (sign_bounds)
constexpr bool K1S_DIRECT(int nc) { return nc <= 12; }

constexpr int FIR_MAX_NE = 128;     // effective taps of the longest table the sign-exact slicer is considered for
constexpr int FIR_MFMA_NC = 48;     // central taps of the matrix-pipe kernel (fir_sign_mfma.hip)
constexpr int FIR_MAX_T = 65280;    // the K1s kernels note open outputs as 16-bit offsets into the segment

// The thresholds of one central-tap count, as a K1s launch takes them: FirLaunch (kernels.h) starts with these.
struct FirThresholds {
    int NC = 12;                    // central taps used: 12, 40 or 48 -- te[(NE-NC)/2 .. +NC)
    int T = 0;                      // outputs per wave, a whole number of the kernel's quantum (plan_fir sets it per call)
    float eps = 0;                  // |central sum| > eps certifies the sign (fir_slice.hip's order of operations)
    float fscale = 0;               // K1s direct form: > 0 = a power of two the central taps are scaled by so that the certified distance
                                    //   is |y'| >= 2.0 and one v_alignbit_b32 gathers sign and exponent bit (fir_sign_kernel FL2); eps is then unused
    float eps_pk = 0;               // the bound for the transposed sum's order of operations (fir_sign_pk.hip)
    // The same bound in two parts, for the kernels that scale it with the largest |x| they have SEEN: eps = eps_seen * M / 32768 +
    // eps_ahead.  The last J0 taps of a reference window multiply samples that lie up to J0 rows beyond the newest one the
    // central sum has loaded; their share of the bound keeps X = 32768 (it is tiny: those taps are) and everything else
    // scales with the maximum M over the rows behind.
    float eps_seen = 0, eps_ahead = 0;
    // fir_sign_pk.hip: the same per output position in its 16-row group: the group's later rows are under the running maximum
    // too, so an output that completes k rows before the group's end has k rows fewer "ahead" ([0..3]: k >= 6, 4, 2, 0)
    float eps_seen_k[4] = {}, eps_ahead_k[4] = {};
};

struct SignBounds {
    bool ok = false;                // the table admits K1s: symmetric, at most FIR_MAX_NE effective taps, bound < 2
    FirThresholds at_nc;            // for the smallest of 12, 48 central taps whose bound stays below 2; T is left 0
    bool ok40 = false;              // 40 central taps pass as well: the packed kernel's alternative where at_nc.NC is 48
    FirThresholds at_40;            //   (eps is at_nc's: only eps_pk and the split are the 40-tap kernel's)
    // the matrix pipe (fir_sign_mfma.hip): the 48 central taps as 24-bit integers tq = round(S t), and the threshold in
    // units of y' = floor(sum tq x / 256): per unit of the largest |x| in reach of a window, absolute
    bool mfma_ok = false;
    float mfma_seen_u = 0.0f, mfma_abs_u = 0.0f;
    int tq[FIR_MFMA_NC] = {};
    long tq_sum = 0;
    double S = 0.0;
};

// te: the NE effective taps (the table without its exactly-zero ends).  NE > FIR_MAX_NE: not admitted, te is not read.
SignBounds sign_bounds(const float *te, int NE);

// The option values the decision depends on (gnuais_batch_set_option)
struct FirOptions {
    int fir_variant = 3;            // 3 sign-exact slicer where the table admits it; 0 the exact ordered sum for every sample
    int fir_T = 512;                // outputs per wave asked for
    int fir_pk_taps = 0;            // 0: 40 central taps where the table allows them; 48: never 40
    int fir_flag2 = 1;              // the direct-form K1s gathers sign and threshold bit with one instruction per output (FL2)
    int fir_mfma = 1;               // long tables run their inner segments on the matrix pipe where the batch allows it
};

// What the options select for a table, independent of any call: gnuais_batch_info() reports exactly this and
// plan_fir() starts from it, so the two cannot disagree.
struct SignChoice {
    bool exact = false;             // K1s runs (calls that ask for the filter's floats aside)
    FirThresholds th;               // the central-tap count in use and its thresholds; fscale 0 where FL2 is off
    float eps = 0.0f;               // the certified distance: FL2's power of two where it is in use, th.eps otherwise
    bool matrix_pipe = false;       // the batch is ELIGIBLE for the matrix pipe; a call takes it when its length allows (plan_fir)
};
SignChoice sign_choice(const SignBounds &sb, const FirOptions &o, int N);

struct FirShape { int N, NT, NE, d; };      // channels, taps, effective taps, NT - first effective tap

// A launch's T must be a whole number of its kernel's quantum.  The kernel files derive these from their unrolled bodies
// (launch_fir_sign_quantum, launch_fir_sign_pk_quantum, launch_fir_sign_mfma's 128) and static_assert the values here.
constexpr int FIR_Q_SIGN12 = 128, FIR_Q_SIGN48 = 384, FIR_Q_PK40 = 640, FIR_Q_PK48 = 384, FIR_Q_MFMA = 128;

enum class FirKernel {
    GENERIC,                        // any table: the exact sum, history and peaks by helper launches
    SCALAR32,                       // 32 effective taps: the exact sum for every sample
    SIGN,                           // K1s, fir_slice.hip
    SIGN_PACKED,                    // K1s on register pairs, 40 / 48 central taps (fir_sign_pk.hip)
    SIGN_PACKED_MFMA                // the packed kernel for the call's first `head` outputs, the matrix pipe for the rest
};

struct FirPlan {
    FirKernel kernel = FirKernel::GENERIC;
    FirThresholds th;               // what the launch starts with
    int head = 0;                   // SIGN_PACKED_MFMA: outputs of the packed launch; the matrix-pipe launch's eps_seen / eps_ahead:
    float mfma_seen_u = 0.0f, mfma_abs_u = 0.0f;
};
// dump: the call asks for the filter's floats (exact kernels only)
FirPlan plan_fir(const SignBounds &sb, const FirOptions &o, const FirShape &s, int len, bool dump);

} // namespace gnuais
