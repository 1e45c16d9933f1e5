// channeliser_kernels.inc -- the text of the channeliser's three kernels, included once by channeliser.hip (int16 input)
// and once by channeliser_fmt.hip (the other sample formats) inside namespace gnuais, behind channeliser_body.h.  The
// includer names the kernels and says where the format comes from:
//   CHAN_FAST_TEMPLATE   the fast form's template head (K and NA; the format as well where it is a parameter)
//   CHAN_FMT_TEMPLATE    the template head of the direct form and the carry copy (empty, or the format)
//   CHAN_FAST_KERNEL, CHAN_DIRECT_KERNEL, CHAN_CARRY_KERNEL   their names
//   CHAN_F               the format: a constant, or the template parameter
// An include and not a template over a wrapper: the int16 kernels keep their names, channeliser_kernel<K, NA>, and
// their instruction streams, which a call through an inlined body does not (registers and schedule move).  The forms
// are described at the top of channeliser.hip.

// the fast form.  grid: 1-D, block b = (segment b / n_groups, stream group b % n_groups); 64 threads (one wave),
// thread = one stream.
CHAN_FAST_TEMPLATE
__global__ __launch_bounds__(64) void CHAN_FAST_KERNEL(ChanLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int rows = a.len / a.D;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const int D = a.D, M = a.M, T = a.T, NP = (D + 1) / 2;
    const void *__restrict__ in = a.in;
    const uint32_t *__restrict__ hist = a.hist;

    int p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = phase_at(a.ph0[k], (r0 - NA + 1) * D, a.per[k]);

    int acc_r[K][NA], acc_i[K][NA];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < NA; ++j) acc_r[k][j] = acc_i[k][j] = 0;

    const size_t N = (size_t) M * K;
    for (int g = r0 - NA + 1; g < r1; ++g) {
        const int t0 = g * D;
        for (int q = 0; q < NP; ++q) {
            const int t = t0 + 2 * q;
            const bool two = 2 * q + 1 < D;
            WideRaw w0, w1;                             // both loads first, then the conversions
            wide_pair_at<CHAN_F>(in, hist, M, T, t, s, two, w0, w1);
            const uint32_t x0 = wide_word<CHAN_F>(w0), x1 = wide_word<CHAN_F>(w1);
            uint32_t pr[K], pi[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t *tab = a.mix + a.off[k];
                int m0r, m0i, m1r = 0, m1i = 0;
                mix(x0, tab[p[k]], m0r, m0i);
                if (++p[k] == a.per[k]) p[k] = 0;
                if (two) {
                    mix(x1, tab[p[k]], m1r, m1i);
                    if (++p[k] == a.per[k]) p[k] = 0;
                }
                pr[k] = pack2(m0r, m1r);
                pi[k] = pack2(m0i, m1i);
            }
            const uint32_t *hp = a.poly + (size_t) q * NA;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const uint32_t h = hp[j];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    acc_r[k][j] = dot2(pr[k], h, acc_r[k][j]);
                    acc_i[k][j] = dot2(pi[k], h, acc_i[k][j]);
                }
            }
        }
        if (g >= r0) {
            uint32_t w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = pack2(sat16((acc_r[k][0] + 16384) >> 15), sat16((acc_i[k][0] + 16384) >> 15));
            using V = typename OutVec<K>::T;
            *reinterpret_cast<V *>(a.out + (size_t) g * N + (size_t) s * K) = OutVec<K>::make(w);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int j = 0; j + 1 < NA; ++j) {
                acc_r[k][j] = acc_r[k][j + 1];
                acc_i[k][j] = acc_i[k][j + 1];
            }
            acc_r[k][NA - 1] = acc_i[k][NA - 1] = 0;
        }
    }
}

// the direct form.  grid: x = (segment, stream group) as above, y = offset k; thread = one stream at offset k.
CHAN_FMT_TEMPLATE
__global__ __launch_bounds__(64) void CHAN_DIRECT_KERNEL(ChanLaunch a)
{
    const int grp = (int) (blockIdx.x % (unsigned) a.n_groups);
    const int seg = (int) (blockIdx.x / (unsigned) a.n_groups);
    const int k = (int) blockIdx.y;
    const int s = grp * 64 + (int) threadIdx.x;
    if (s >= a.M) return;
    const int rows = a.len / a.D;
    const int r0 = seg * a.seg_rows;
    if (r0 >= rows) return;
    const int r1 = min(r0 + a.seg_rows, rows);
    const int D = a.D, M = a.M, T = a.T, P = a.per[k];
    const uint32_t *tab = a.mix + a.off[k];
    for (int m = r0; m < r1; ++m) {
        const int e = m * D + D - 1;
        int p = phase_at(a.ph0[k], e, P);
        int ar = 0, ai = 0;
        for (int j = 0; j < T; ++j) {
            int mr, mi;
            mix(wide_at<CHAN_F>(a.in, a.hist, M, T, e - j, s), tab[p], mr, mi);
            const int h = (int) a.taps[j];
            ar += h * mr;
            ai += h * mi;
            p = (p == 0) ? P - 1 : p - 1;
        }
        a.out[(size_t) m * M * a.K + (size_t) s * a.K + k] = pack2(sat16((ar + 16384) >> 15), sat16((ai + 16384) >> 15));
    }
}

// the new carry, as converted words whatever the format: hist_out[i] = the call's wide sample len-(T-1)+i, from the input or
// (short calls) the old carry
CHAN_FMT_TEMPLATE
__global__ __launch_bounds__(256) void CHAN_CARRY_KERNEL(const void *__restrict__ in, const uint32_t *__restrict__ hist_in,
                                                         uint32_t *__restrict__ hist_out, int M, int T, int len)
{
    const long long idx = (long long) blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long) (T - 1) * M) return;
    const int i = (int) (idx / M), s = (int) (idx % M);
    const int t = len - (T - 1) + i;
    hist_out[idx] = t >= 0 ? wide_word<CHAN_F>(wide_load<CHAN_F>(in, (size_t) t * M + s)) : hist_in[(size_t) (len + i) * M + s];
}
